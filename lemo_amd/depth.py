"""Kinect depth frames to body scans on the device (``csrc/depth_scan_kernels.hip``): the reference's ``Projection.create_scan``
(temp_prox/projection_utils.py:35-90) and the truncate / pad / mean its loader applies per frame (temp_prox/data_parser_slide.py:
283-323), for a whole window of frames in one launch chain.

    proj = DepthProjection(calib_dir)                                   # IR.json + Color.json; builds the ray table once per frame size
    out = proj.create_scan(mask, depth)                                 # mask uint8 [B, 1080, 1920], depth float32 [B, 424, 512]
    out['scan'], out['scan_point_num'], out['init_trans']               # [B, 20000, 3], int32 [B], [B, 3]: what scan_terms takes

What is restated rather than run: OpenCV is not part of this project's environment.  ``cv2.undistortPoints`` (5 fixed-point
iterations, its default) and ``cv2.projectPoints`` (Rodrigues rotation, pinhole division, ``k = (k1, k2, p1, p2, k3)``) follow
OpenCV's documented distortion model; agreement with OpenCV itself is NOT confirmed by a run.  Everything that depends on the
calibration alone -- the undistorted ray of every depth pixel, the colour camera's rotation matrix -- is computed once on the host in
float64 and rounded to float32; everything that depends on the frame runs in the kernels.  One difference to the reference, on
purpose: with ``mask_on_color=False`` the reference zeroes the caller's depth image in place (projection_utils.py:56); here the
caller's depth is left as it is.  Everything takes and returns device tensors and nothing waits for the device; there is no CPU path.
``Projection`` is the drop-in with the reference's method names (numpy in, numpy out, one frame per call).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import ptr

MAX_BATCH = 1024                # lemo_depth_scan's limits
MAX_PIXELS = 1 << 22
MAX_SCAN = 1 << 20
MAX_COLOR_SIDE = 32768
DEFAULT_COLOR = (1.00, 0.75, 0.80)
UNDISTORT_ITERS = 5             # cv2.undistortPoints' default iteration count


def rodrigues(r) -> np.ndarray:
    """rotation vector [3] -> float64 rotation matrix [3, 3] (cv2.Rodrigues)"""
    r = np.asarray(r, np.float64).reshape(3)
    th = float(np.linalg.norm(r))
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def undistorted_rays(camera_mtx, k, H: int, W: int, iters: int = UNDISTORT_ITERS) -> np.ndarray:
    """float64 [H, W, 2]: the undistorted normalised coordinate of every pixel centre (u, v), by ``iters`` fixed-point iterations
    from ((u - cx) / fx, (v - cy) / fy), as cv2.undistortPoints without R / P"""
    M, k = np.asarray(camera_mtx, np.float64), np.asarray(k, np.float64).reshape(-1)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    x0, y0 = (u - M[0, 2]) / M[0, 0], (v - M[1, 2]) / M[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x)
        dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x, y], -1)


def _cam_dict(cam, name: str, need) -> Dict[str, np.ndarray]:
    shapes = {'camera_mtx': (3, 3), 'k': (5,), 'view_mtx': (3, 4), 'R': (3,), 'T': (3,)}
    out = {}
    for key in need:
        if key not in cam:
            raise ValueError(f'{name} has no {key!r}')
        a = np.asarray(cam[key], np.float64)
        if a.size != int(np.prod(shapes[key])) or not np.all(np.isfinite(a)):
            raise ValueError(f'{name}[{key!r}] must hold {shapes[key]} finite numbers, got shape {a.shape}')
        out[key] = a.reshape(shapes[key])
    return out


class DepthProjection:
    """The two Kinect cameras of a PROX recording.  ``calib_dir`` holds ``IR.json`` and ``Color.json`` (the reference's calibration
    files), or pass the two dicts: ``depth_cam`` needs ``camera_mtx``, ``k``, ``view_mtx``; ``color_cam`` needs those and ``R``
    (Rodrigues vector), ``T``.  ``color_size`` = (rows, columns) of the colour image, 1080 x 1920 for PROX."""

    def __init__(self, calib_dir: Optional[str] = None, depth_cam=None, color_cam=None, color_size: Tuple[int, int] = (1080, 1920),
                 device='cuda', _lib: Optional[_hip.HipLib] = None):
        if calib_dir is not None:
            if depth_cam is not None or color_cam is not None:
                raise ValueError('give calib_dir or the two camera dicts, not both')
            with open(os.path.join(calib_dir, 'IR.json')) as f:
                depth_cam = json.load(f)
            with open(os.path.join(calib_dir, 'Color.json')) as f:
                color_cam = json.load(f)
        if depth_cam is None or color_cam is None:
            raise ValueError('DepthProjection needs calib_dir or both depth_cam and color_cam')
        self.depth_cam = _cam_dict(depth_cam, 'depth_cam', ('camera_mtx', 'k', 'view_mtx'))
        self.color_cam = _cam_dict(color_cam, 'color_cam', ('camera_mtx', 'k', 'view_mtx', 'R', 'T'))
        cH, cW = int(color_size[0]), int(color_size[1])
        if not (1 <= cH <= MAX_COLOR_SIDE and 1 <= cW <= MAX_COLOR_SIDE):
            raise ValueError(f'color_size must be (rows, columns) within 1 .. {MAX_COLOR_SIDE}, got {color_size}')
        self.color_size = (cH, cW)
        self.device = torch.device(device)
        self._lib = _lib
        self.Rc = rodrigues(self.color_cam['R'])                 # float64, once
        self._calib: Dict[Tuple[int, int], Tuple[_hip.DepthCalib, torch.Tensor]] = {}
        self._proj_const: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}      # project_points' R^T and T on the device, per camera

    # ------------------------------------------------------------------------------------------------ host constants
    def _library(self) -> _hip.HipLib:
        return self._lib or _hip.get_lib()

    def rays(self, H: int, W: int) -> torch.Tensor:
        """float32 [H, W, 2] on the device: the ray table of an H x W depth frame (built on first use, then kept)"""
        return self._calibration(H, W)[1]

    def _calibration(self, H: int, W: int):
        key = (int(H), int(W))
        if key not in self._calib:
            rays = torch.from_numpy(undistorted_rays(self.depth_cam['camera_mtx'], self.depth_cam['k'], H, W).astype(np.float32)).to(self.device)
            c, M = _hip.DepthCalib(), self.color_cam['camera_mtx']
            c.rays = ptr(rays)
            c.view_d[:] = self.depth_cam['view_mtx'].reshape(-1).tolist()
            c.Rc[:] = self.Rc.reshape(-1).tolist()
            c.Tc[:] = self.color_cam['T'].tolist()
            c.fx, c.fy, c.cx, c.cy = float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2])
            c.k[:] = self.color_cam['k'].tolist()
            c.view_c[:] = self.color_cam['view_mtx'].reshape(-1).tolist()
            c.cH, c.cW = self.color_size
            self._calib[key] = (c, rays)
        return self._calib[key]

    # ------------------------------------------------------------------------------------------------ argument checks
    def _depth(self, lib, depth, raw: bool) -> torch.Tensor:
        if not isinstance(depth, torch.Tensor):
            raise ValueError('depth must be a torch tensor on the device (there is no CPU path)')
        want = torch.uint16 if raw else torch.float32
        if depth.dtype != want:
            raise ValueError(f'depth must be {want} (raw={raw}), got {depth.dtype}')
        if depth.dim() != 3 or min(depth.shape) < 1:
            raise ValueError(f'depth must be [B, H, W] with at least one frame and one pixel, got {tuple(depth.shape)}')
        if depth.device != self.device:
            raise ValueError(f'depth is on {depth.device}, the projection on {self.device}')
        B, H, W = depth.shape
        if B > MAX_BATCH or H * W > MAX_PIXELS:
            raise ValueError(f'at most {MAX_BATCH} frames of {MAX_PIXELS} pixels, got {tuple(depth.shape)}')
        try:
            _hip.check_device(lib, depth)
        except _hip.LemoHipError as e:                            # a CPU tensor for the product library: a refusal like the others
            raise ValueError(str(e)) from None
        return depth.detach().contiguous()

    @staticmethod
    def _options(flip, depth_scale):
        depth_scale = float(depth_scale)
        if not np.isfinite(depth_scale):
            raise ValueError(f'depth_scale must be finite, got {depth_scale}')
        return int(bool(flip)), depth_scale

    # ------------------------------------------------------------------------------------------------ the reference's methods
    def unproject_depth_image(self, depth: torch.Tensor, raw: bool = False, flip: bool = False, depth_scale: float = 1e-3) -> torch.Tensor:
        """``depth`` [B, H, W] (float32 metres, or uint16 with ``raw``) -> float32 [B, H, W, 3]: projection_utils.py:35-48 per frame"""
        lib = self._library()
        d = self._depth(lib, depth, raw)
        flip, depth_scale = self._options(flip, depth_scale)
        B, H, W = d.shape
        cal, _ = self._calibration(H, W)
        points = torch.empty(B, H, W, 3, dtype=torch.float32, device=self.device)
        lib.check(lib.depth_unproject(ptr(d), int(raw), flip, depth_scale, C.byref(cal), B, H, W, ptr(points), lib.stream(self.device)),
                  'depth_unproject')
        return points

    def project_points(self, points: torch.Tensor, cam: str = 'color') -> torch.Tensor:
        """``points`` float32 [.., 3] on the device -> float32 [.., 2]: the (u, v) pixel coordinates ``cv2.projectPoints`` gives with
        the colour camera's R, T, camera_mtx, k (projection_utils.py:50-52), not rounded.  A utility in torch operations (the scan
        kernels project for themselves); ``cam='depth'`` projects with the IR camera's intrinsics and no rotation."""
        if cam not in ('color', 'depth'):
            raise ValueError(f"cam must be 'color' or 'depth', got {cam!r}")
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() < 1 or points.shape[-1] != 3:
            raise ValueError('points must be a float32 tensor [.., 3] on the device')
        if points.device != self.device:
            raise ValueError(f'points are on {points.device}, the projection on {self.device}')
        c = self.color_cam if cam == 'color' else self.depth_cam
        if cam not in self._proj_const:                           # uploaded once per camera, like the ray table
            R = self.Rc if cam == 'color' else np.eye(3)
            T = c['T'] if cam == 'color' else np.zeros(3)
            t = lambda a: torch.from_numpy(np.array(a, np.float32, order='C')).to(self.device)
            self._proj_const[cam] = (t(R.T), t(T))
        Rt, T = self._proj_const[cam]
        q = points @ Rt + T
        x, y = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        k, M = [float(v) for v in c['k']], c['camera_mtx']
        r2 = x * x + y * y
        cd = 1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
        a1, a2, a3 = 2.0 * x * y, r2 + 2.0 * x * x, r2 + 2.0 * y * y
        xd, yd = x * cd + k[2] * a1 + k[3] * a2, y * cd + k[2] * a3 + k[3] * a1
        return torch.stack([float(M[0, 0]) * xd + float(M[0, 2]), float(M[1, 1]) * yd + float(M[1, 2])], -1)

    def create_scan(self, mask: torch.Tensor, depth: torch.Tensor, mask_on_color: bool = True, coord: Optional[str] = 'color', TH: float = 1e-2,
                    S: int = 20000, raw: bool = False, flip: bool = False, depth_scale: float = 1e-3, return_pixels: bool = False,
                    out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """``depth`` [B, H, W]: float32 metres, or with ``raw`` the uint16 of the recording (``d = raw / 8 * depth_scale``,
        data_parser_slide.py:285-287); ``flip`` reads it mirrored left-right (:288-289).  ``mask`` uint8 / bool: with
        ``mask_on_color`` [B, rows, columns] of the colour image, looked up where each point projects (0 = keep); without, [B, H, W]
        at depth resolution, the depth counting as 0 where it is non-zero.  A pixel survives iff its depth is finite, the z of its
        point exceeds ``TH`` and -- ``mask_on_color`` only -- it projects into the colour image onto a zero of the mask.  ``coord``:
        'color' gives points in the colour camera's frame, None the unprojected ones.

        -> ``scan`` float32 [B, S, 3]: the first ``S`` surviving points of each frame in row-major pixel order, zeros behind them
        (:319-323); ``scan_point_num`` int32 [B] = min(n_valid, S), what ``scan_terms`` / ``ProxTemporalFitter`` take; ``n_valid``
        int32 [B]: all survivors (the reference's uncapped count); ``init_trans`` float32 [B, 3]: the mean of ALL surviving points
        (:306), NaN for a frame without any; with ``return_pixels`` also ``points`` [B, H, W, 3] and ``valid`` uint8 [B, H, W].  The
        scan holds exactly the bits of ``points[valid]``.  ``out``: a float32 [B, S, 3] tensor to write the scan into (it needs no
        initialisation).  Deterministic; nothing waits for the device; bad arguments raise ``ValueError`` before any launch."""
        lib = self._library()
        d = self._depth(lib, depth, raw)
        flip, depth_scale = self._options(flip, depth_scale)
        B, H, W = d.shape
        if coord not in ('color', None):
            raise ValueError(f"coord must be 'color' or None, got {coord!r}")
        TH, S = float(TH), int(S)
        if not np.isfinite(TH):
            raise ValueError(f'TH must be finite, got {TH}')
        if not 1 <= S <= MAX_SCAN:
            raise ValueError(f'S must lie in 1 .. {MAX_SCAN}, got {S}')
        want = (B,) + (self.color_size if mask_on_color else (H, W))
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError('mask must be a uint8 / bool tensor on the device')
        if tuple(mask.shape) != want or mask.device != self.device:
            raise ValueError(f'mask must be {want} on {self.device} (mask_on_color={bool(mask_on_color)}), got {tuple(mask.shape)} on {mask.device}')
        m = mask.contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (B, S, 3) or out.device != self.device \
                    or not out.is_contiguous():
                raise ValueError(f'out must be a contiguous float32 tensor [{B}, {S}, 3] on {self.device}')
        nbytes = int(lib.depth_scan_ws_bytes(B, H, W))
        if nbytes < 0:
            raise ValueError(f'create_scan: shape {tuple(d.shape)} is not taken')
        cal, _ = self._calibration(H, W)
        dev = self.device
        scan = out if out is not None else torch.empty(B, S, 3, dtype=torch.float32, device=dev)
        spn, n_valid = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        init_trans = torch.empty(B, 3, dtype=torch.float32, device=dev)
        points = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if return_pixels else None
        valid = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if return_pixels else None
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        lib.check(lib.depth_scan(ptr(d), int(raw), flip, depth_scale, ptr(m), int(bool(mask_on_color)), int(coord == 'color'), TH, C.byref(cal),
                                 B, H, W, S, ptr(scan), ptr(spn), ptr(n_valid), ptr(init_trans), ptr(points), ptr(valid), ptr(ws), nbytes,
                                 lib.stream(dev)), 'depth_scan')
        res = {'scan': scan, 'scan_point_num': spn, 'n_valid': n_valid, 'init_trans': init_trans}
        if return_pixels:
            res.update(points=points, valid=valid)
        return res


class Projection:
    """Drop-in for the reference's ``Projection`` (temp_prox/projection_utils.py:23): the same method names, numpy in and numpy out,
    one frame per call, computed on the device.  ``create_scan`` returns ``{'points', 'colors'}`` with ``colors`` the default-colour
    tile; a ``color_im`` raises ``NotImplementedError`` (colours from the image, ``align_color2depth`` and ``align_depth2color`` are not
    provided).  Unlike the reference, ``depth_im`` is not modified.  An empty ``depth_im`` returns ``{'v': []}`` as the reference does
    (projection_utils.py:57-58)."""

    def __init__(self, calib_dir: Optional[str] = None, depth_cam=None, color_cam=None, color_size: Tuple[int, int] = (1080, 1920), device='cuda',
                 _lib: Optional[_hip.HipLib] = None):
        self._p = DepthProjection(calib_dir, depth_cam, color_cam, color_size, device, _lib)
        self.depth_cam, self.color_cam = self._p.depth_cam, self._p.color_cam

    def _frame(self, a, dtype, name: str) -> torch.Tensor:
        a = np.asarray(a)
        if a.ndim != 2 or a.size == 0:
            raise ValueError(f'{name} must be one frame [rows, columns], got shape {a.shape}')
        return torch.from_numpy(np.array(a, dtype, order='C')[None]).to(self._p.device)      # a copy: the caller's array is never written

    def unproject_depth_image(self, depth_image, cam=None) -> np.ndarray:
        if cam is not None and cam is not self.depth_cam:
            raise NotImplementedError('unproject_depth_image is provided for the depth camera only')
        return self._p.unproject_depth_image(self._frame(depth_image, np.float32, 'depth_image'))[0].cpu().numpy().astype(np.float64)

    def projectPoints(self, v, cam=None) -> np.ndarray:
        if cam is not None and cam is not self.color_cam:
            raise NotImplementedError('projectPoints is provided for the colour camera only')
        pts = torch.from_numpy(np.array(np.asarray(v).reshape(-1, 3), np.float32, order='C')).to(self._p.device)
        return self._p.project_points(pts).cpu().numpy().astype(np.float64)

    def create_scan(self, mask, depth_im, color_im=None, mask_on_color: bool = False, coord: Optional[str] = 'color', TH: float = 1e-2,
                    default_color=DEFAULT_COLOR) -> Dict[str, np.ndarray]:
        if color_im is not None:
            raise NotImplementedError('colours from color_im are not provided; pass color_im=None')
        if np.asarray(depth_im).size == 0:
            return {'v': []}
        d = self._frame(depth_im, np.float32, 'depth_im')
        if d.shape[1] * d.shape[2] > MAX_SCAN:
            raise ValueError(f'the drop-in takes frames of at most {MAX_SCAN} pixels, got {tuple(d.shape[1:])}')
        m = np.asarray(mask)
        m = self._frame(m != 0 if m.dtype != np.uint8 else m, np.uint8, 'mask')
        out = self._p.create_scan(m, d, mask_on_color=mask_on_color, coord=coord, TH=TH, S=d.shape[1] * d.shape[2])
        n = int(out['n_valid'][0])
        points = out['scan'][0, :n].cpu().numpy().astype(np.float64)
        return {'points': points, 'colors': np.tile(np.asarray(default_color, np.float64), [n, 1])}
