"""Occlusion masks of a PROX recording on the device (``csrc/occlusion_kernels.hip``).

The reference's ``utils/get_occlusion_mask.py`` renders the static scene once and the fitted SMPL-X body for every frame with
pyrender at 1920 x 1080, and marks a joint occluded where the scene lies more than 0.1 m in front of the body at the joint's
pixel (``mask_joint.npy``; its marker twin ``mask_markers.npy`` [T, 67] is what ``ProxWindowEngine(marker_mask=...)``,
``pipeline.prox_window_setup`` and ``infill_train.load_prox_mask_clips`` consume).  Here

    scene = SceneDepth(scene_verts, scene_faces, cam2world)                  # one raster; scene.depth [H, W] on the device
    masker = OcclusionMasker(scene, body_model.faces)
    out = body_model(**fitted_params)                                        # T frames, camera coordinates
    joint_mask = masker.joints(out)                                          # [T, 25], 1 = visible   (mask_joint.npy)
    marker_mask = masker.markers(out, load_vertex_ids()['markers67'])        # [T, 67]                (mask_markers.npy)

The body is never rendered: its depth is evaluated at the queried pixels only.  Everything takes and returns device tensors.

What is restated rather than run: pyrender is not part of this project's environment, so the raster follows what its
``IntrinsicsCamera`` projection and OpenGL's sampling rule say on paper -- pixel [y][x] samples the ray through (x + 0.5, y + 0.5),
depth is the linear camera-space Z of the nearest hit with 0.05 <= Z <= 100, 0 where nothing is hit.  ``cull_backface=True`` is an
ASSUMPTION from reading pyrender's renderer (it enables ``GL_CULL_FACE`` for materials that are not ``doubleSided``, which covers
both materials of the reference script); it has not been confirmed by a run, so both settings are supported and tested.
pyrender reads Z back from a 24-bit depth buffer (steps of about 1e-5 m at 3 m); this module returns the exact fp32 Z.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _hip
from ._hip import ptr

# get_occlusion_mask.py:111-116 (render) and :132-134 (projection of the joints: fy differs from the render's)
PROX_RENDER = dict(W=1920, H=1080, fx=1060.53, fy=1060.38, cx=951.30, cy=536.77)
PROX_PROJ = dict(proj_fx=1060.53, proj_fy=1060.53)
MAX_POINTS = 128
MAX_FRAMES = 65535
MAX_SIDE = 32768


def _mesh(lib, verts, faces, batched: bool):
    """validated (verts float32 contiguous, faces int32 contiguous); faces may come as a numpy array (a model's ``faces``)"""
    if not isinstance(verts, torch.Tensor):
        raise ValueError('vertices must be a torch tensor on the device')
    _hip.check_device(lib, verts)
    want = 3 if batched else 2
    if verts.dim() != want or verts.shape[-1] != 3 or verts.shape[-2] < 1 or verts.dtype != torch.float32:
        raise ValueError(f'vertices must be float32 {"[T, V, 3]" if batched else "[V, 3]"}, got {verts.dtype} {tuple(verts.shape)}')
    if not isinstance(faces, torch.Tensor):
        f = np.asarray(faces)
        if f.dtype.kind not in 'iu':
            raise ValueError(f'faces must be integers, got {f.dtype}')
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f'faces must be [F, 3], got {f.shape}')
        if f.min() < 0 or f.max() >= verts.shape[-2]:
            raise ValueError(f'faces name vertices {int(f.min())} .. {int(f.max())}, the mesh has {verts.shape[-2]}')
        faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(verts.device)
    else:
        _hip.check_device(lib, faces)
        if faces.dtype != torch.int32:
            raise ValueError(f'a faces tensor must be int32, got {faces.dtype}')
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError(f'faces must be [F, 3], got {tuple(faces.shape)}')
        if faces.device != verts.device:
            raise ValueError('faces and vertices are on different devices')
    return verts.contiguous(), faces.contiguous()


def _cam(W, H, fx, fy, cx, cy, znear, zfar, cull_backface) -> _hip.OcclCam:
    W, H = int(W), int(H)
    if W < 1 or H < 1 or W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError(f'image size must be 1 .. {MAX_SIDE} on each side, got {W} x {H}')
    vals = [float(v) for v in (fx, fy, cx, cy, znear, zfar)]
    if not all(np.isfinite(vals)) or vals[0] <= 0 or vals[1] <= 0 or vals[4] <= 0 or vals[5] < vals[4]:
        raise ValueError('intrinsics and depth range must be finite, fx, fy, znear > 0 and zfar >= znear')
    return _hip.OcclCam(*vals, W, H, int(bool(cull_backface)))


def _xf(transform) -> Optional[C.Array]:
    """[3 or 4, 4] rigid transform -> the 12 floats the raster applies on load"""
    if transform is None:
        return None
    m = transform.detach().cpu().numpy() if isinstance(transform, torch.Tensor) else np.asarray(transform)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        raise ValueError(f'a transform is a finite [3, 4] or [4, 4] matrix, got {m.shape}')
    return (C.c_float * 12)(*np.asarray(m[:3], np.float32).reshape(-1).tolist())


def render_depth(verts: torch.Tensor, faces, transform=None, W: int = 1920, H: int = 1080, fx: float = 1060.53, fy: float = 1060.38,
                 cx: float = 951.30, cy: float = 536.77, znear: float = 0.05, zfar: float = 100.0, cull_backface: bool = True,
                 _lib: Optional[_hip.HipLib] = None) -> torch.Tensor:
    """Depth image [H, W] of a triangle mesh (verts [V, 3] float32, faces [F, 3]) on the device: camera-space Z of the nearest
    surface per pixel, 0 where there is none.  ``transform``: rigid [4, 4] applied to the vertices first (world -> camera).
    ``cull_backface``: see the module docstring -- an assumption about pyrender, not a confirmed fact."""
    lib = _lib or _hip.get_lib()
    verts, faces = _mesh(lib, verts, faces, batched=False)
    cam = _cam(W, H, fx, fy, cx, cy, znear, zfar, cull_backface)
    xf = _xf(transform)
    depth = torch.empty(cam.H, cam.W, dtype=torch.float32, device=verts.device)
    lib.check(lib.depth_raster(ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], xf, C.byref(cam), ptr(depth),
                               lib.stream(verts.device)), 'depth_raster')
    return depth


class SceneDepth:
    """The static scene rendered once (get_occlusion_mask.py:111-147): ``scene_verts`` [V, 3] in world coordinates,
    ``cam2world`` [4, 4] as PROX's ``cam2world/<scene>.json`` holds it (its inverse is applied, :124-125).  ``.depth`` [H, W]."""

    def __init__(self, scene_verts: torch.Tensor, scene_faces, cam2world=None, W: int = 1920, H: int = 1080, fx: float = 1060.53,
                 fy: float = 1060.38, cx: float = 951.30, cy: float = 536.77, znear: float = 0.05, zfar: float = 100.0,
                 cull_backface: bool = True, _lib: Optional[_hip.HipLib] = None):
        self.lib = _lib or _hip.get_lib()
        world2cam = None
        if cam2world is not None:
            m = cam2world.detach().cpu().numpy() if isinstance(cam2world, torch.Tensor) else np.asarray(cam2world)
            if m.shape != (4, 4) or not np.all(np.isfinite(m)):
                raise ValueError(f'cam2world is a finite [4, 4] matrix, got {m.shape}')
            world2cam = np.linalg.inv(m.astype(np.float64))
        self.world2cam = world2cam
        self.params = dict(W=int(W), H=int(H), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), znear=float(znear),
                           zfar=float(zfar), cull_backface=bool(cull_backface))
        self.depth = render_depth(scene_verts, scene_faces, world2cam, _lib=self.lib, **self.params)
        self.device = self.depth.device


class OcclusionMasker:
    """The per-frame half (get_occlusion_mask.py:170-201).  ``body_faces`` [F, 3]; ``thresh``: metres the scene must lie in front
    of the body (:198); ``proj_fx / proj_fy``: the intrinsics the POINTS are projected with (:132-134 sets both to 1060.53 although
    the render uses fy = 1060.38 -- kept apart on purpose).  ``cull_backface`` (default: the scene's) applies to the body mesh.
    ``chunk`` frames go into one launch; any number of frames can be passed."""

    def __init__(self, scene: SceneDepth, body_faces, thresh: float = 0.1, proj_fx: float = 1060.53, proj_fy: float = 1060.53,
                 cull_backface: Optional[bool] = None, chunk: int = 512):
        if not isinstance(scene, SceneDepth):
            raise ValueError('scene must be a SceneDepth')
        self.scene, self.lib, self.device = scene, scene.lib, scene.device
        if not 1 <= int(chunk) <= MAX_FRAMES:
            raise ValueError(f'chunk must be 1 .. {MAX_FRAMES} frames')
        vals = [float(thresh), float(proj_fx), float(proj_fy)]
        if not all(np.isfinite(vals)) or vals[1] <= 0 or vals[2] <= 0:
            raise ValueError('thresh must be finite and proj_fx, proj_fy finite and positive')
        self.thresh, self.proj_fx, self.proj_fy, self.chunk = vals[0], vals[1], vals[2], int(chunk)
        p = dict(scene.params)
        if cull_backface is not None:
            p['cull_backface'] = bool(cull_backface)
        self._cam = _cam(**p)
        if isinstance(body_faces, torch.Tensor):
            _hip.check_device(self.lib, body_faces)
            if body_faces.dtype != torch.int32 or body_faces.dim() != 2 or body_faces.shape[1] != 3 or body_faces.shape[0] < 1:
                raise ValueError(f'a faces tensor must be int32 [F, 3], got {body_faces.dtype} {tuple(body_faces.shape)}')
            self.faces = body_faces.to(self.device).contiguous()
        else:
            f = np.asarray(body_faces)
            if f.dtype.kind not in 'iu' or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.min() < 0:
                raise ValueError(f'body_faces must be non-negative integers [F, 3], got {f.dtype} {f.shape}')
            self.faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(self.device)
        self._vmin = int(self.faces.max()) + 1                   # once, at construction: vertices the faces need

    def __call__(self, vertices: torch.Tensor, points: torch.Tensor, return_depth: bool = False, return_pixels: bool = False):
        """vertices [T, V, 3], points [T, P <= 128, 3], camera coordinates -> mask [T, P] float32, 1 = visible.
        ``return_depth`` / ``return_pixels`` add the body's depth at each point's pixel [T, P] (0: not covered) and the pixel
        (x, y) [T, P, 2] int32."""
        verts, _ = _mesh(self.lib, vertices, self.faces, batched=True)
        if not isinstance(points, torch.Tensor):
            raise ValueError('points must be a torch tensor on the device')
        _hip.check_device(self.lib, points)
        if points.dim() != 3 or points.shape[-1] != 3 or points.dtype != torch.float32 or points.shape[0] != verts.shape[0]:
            raise ValueError(f'points must be float32 [T = {verts.shape[0]}, P, 3], got {points.dtype} {tuple(points.shape)}')
        T, V, P = verts.shape[0], verts.shape[1], points.shape[1]
        if T < 1 or not 1 <= P <= MAX_POINTS:
            raise ValueError(f'T >= 1 and 1 <= P <= {MAX_POINTS} query points per frame, got T = {T}, P = {P}')
        if V < self._vmin:
            raise ValueError(f'the faces name vertex {self._vmin - 1}, the mesh has {V} vertices')
        if points.device != verts.device or verts.device != self.scene.depth.device:
            raise ValueError('vertices, points and the scene depth must be on one device')
        points = points.contiguous()
        dev = verts.device
        mask = torch.empty(T, P, dtype=torch.float32, device=dev)
        depth = torch.empty(T, P, dtype=torch.float32, device=dev) if return_depth else None
        pix = torch.empty(T, P, 2, dtype=torch.int32, device=dev) if return_pixels else None
        ws = torch.empty(min(T, self.chunk) * P, dtype=torch.int32, device=dev)
        s = self.lib.stream(dev)
        for lo in range(0, T, self.chunk):
            hi = min(T, lo + self.chunk)
            sub = lambda t: None if t is None else ptr(t[lo:hi])
            self.lib.check(self.lib.occlusion_query(ptr(verts[lo:hi]), hi - lo, V, ptr(self.faces), self.faces.shape[0], ptr(points[lo:hi]),
                                                    P, C.byref(self._cam), self.proj_fx, self.proj_fy, ptr(self.scene.depth), self.thresh,
                                                    ptr(ws), sub(mask), sub(depth), sub(pix), s), 'occlusion_query')
        extra = tuple(t for t in (depth, pix) if t is not None)
        return (mask,) + extra if extra else mask

    def joints(self, smplx_output, n: int = 25) -> torch.Tensor:
        """``mask_joint.npy``: the first ``n`` joints of a body-model output of T frames (get_occlusion_mask.py:189-201)"""
        return self(smplx_output.vertices.detach(), smplx_output.joints.detach()[:, :n].contiguous())

    def markers(self, smplx_output, marker_ids) -> torch.Tensor:
        """``mask_markers.npy`` layout [T, len(marker_ids)]: the same rule at ``vertices[:, marker_ids]``"""
        verts = smplx_output.vertices.detach()
        ids = np.asarray(marker_ids, np.int64)
        if ids.ndim != 1 or ids.size < 1 or ids.min() < 0 or ids.max() >= verts.shape[1]:
            raise ValueError('marker_ids must be vertex indices of the body model')
        return self(verts, verts[:, torch.from_numpy(ids).to(verts.device)].contiguous())
