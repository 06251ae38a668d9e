"""Body overlays on the device (``csrc/render_kernels.hip``): the fitted body in the PROX camera view, shaded, over the colour
frame, the 2-D joints on top -- the images the ``render_results`` branch of the reference's
``temp_prox/fit_temp_loadprox_slide.py:622-683`` writes next to its pkl files.

    r = BodyRenderer(body_model.faces)                          # the PROX camera (occlusion.PROX_RENDER)
    out = body_model(**fitted_params)                           # B frames, camera coordinates
    img = r(out.vertices, background=frames, points=joints2d)   # uint8 [B, 1080, 1920, 3] on the device
    n = vertex_normals(out.vertices, body_model.faces)          # [B, V, 3] unit normals

Everything takes and returns device tensors.  ``chunk`` frames go into one set of launches and the workspace (depth keys, face
ids, normals) is sized by ``chunk``, not by the number of frames; the result does not depend on it, bit for bit.

THE RULE BELOW IS THIS PROJECT'S OWN.  pyrender is not part of this project's environment and its metallic-roughness material is
not restated; what is said about pyrender (pixel centres, culling, the light's pose) rests on reading, as in ``occlusion.py``.

1. Normals.  n_v = the sum, over the faces f that contain v in ascending f, of (p1 - p0) x (p2 - p0) -- unnormalised, hence
   area-weighted; unit = n / sqrt(n . n) if n . n > 0, else (0, 0, 0).  Faces that name a vertex outside [0, V) are skipped, as the
   raster skips them.  No float atomics: the vertex -> face adjacency (CSR) is built once per topology on the host, at construction,
   and gathered, so the bits do not depend on the run, the launch shape or ``chunk``.
2. Coverage, depth, face id.  Coverage and depth are exactly ``occlusion.render_depth``'s (the same device functions: the same
   pixel-centre sampling, homogeneous edge functions, near-plane handling without clipping and culling rule), so ``return_depth`` is
   bit for bit what ``render_depth`` returns for that frame.  The face id of a pixel is the lowest-index face among those whose depth
   there equals the nearest.
3. Shading of a covered pixel.  With the winning face's edge functions e0, e1, e2 at the pixel's ray, b_i = e_i / (e0 + e1 + e2)
   (perspective-correct; e0 weighs p0, e1 p1, e2 p2); n = b0 n0 + b1 n1 + b2 n2 of the unit vertex normals; lambert = |n_z| / |n|, 0 if
   |n| = 0 -- a two-sided head light along the viewing axis (the script gives its light the camera's pose);
   shade = min(1, ambient + diffuse lambert); colour_k = base_k shade.
4. Quantisation and compositing.  q = (int)(255 c + 0.5) clamped to 0 .. 255; the same rule quantises a float32 background.  An
   uncovered pixel is the background's pixel, (0, 0, 0) without a background.
5. Points.  x = trunc(u), y = trunc(v), as ``projected_joints.astype(int)``; the pixels (x + i, y + j) with i^2 + j^2 <= r^2 inside
   the image get ``point_color``, over the body; non-finite points are skipped; one colour per call, so the result does not depend
   on order.  THIS IS NOT PIL'S ELLIPSE RULE (``ImageDraw.ellipse`` fills its bounding box's inscribed ellipse, whose edge pixels
   differ); it is a plain integer disc.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _hip
from ._hip import ptr
from .occlusion import MAX_FRAMES, PROX_RENDER, _cam

MAX_RADIUS = 16


def _faces_host(faces) -> np.ndarray:
    """[F, 3] int32 on the host, validated (non-negative integers); a device tensor is copied once"""
    if isinstance(faces, torch.Tensor):
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError(f'a faces tensor must be int32 [F, 3], got {faces.dtype} {tuple(faces.shape)}')
        f = faces.detach().cpu().numpy()
    else:
        f = np.asarray(faces)
        if f.dtype.kind not in 'iu' or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f'faces must be integers [F, 3], got {f.dtype} {f.shape}')
    if f.min() < 0 or f.max() >= 2 ** 30:
        raise ValueError(f'faces name vertices {int(f.min())} .. {int(f.max())}')
    return np.ascontiguousarray(f, np.int32)


def face_adjacency(faces: np.ndarray, V: int):
    """CSR of vertex -> faces: (start [V + 1], face [nnz]) int32; row v lists the faces that contain v in ascending order, each once"""
    F = faces.shape[0]
    v = faces.astype(np.int64).reshape(-1)
    f = np.repeat(np.arange(F, dtype=np.int64), 3)
    pair = np.unique(v * F + f)                               # sorted by (vertex, face); a face that names v twice counts once
    v, f = pair // F, pair % F
    f = f[v < V]
    start = np.zeros(V + 1, np.int64)
    np.add.at(start, v[v < V] + 1, 1)
    return np.cumsum(start).astype(np.int32), np.ascontiguousarray(f, np.int32)


class _Topology:
    """faces and their adjacency on the host; uploaded once per device"""

    def __init__(self, faces):
        self.faces = _faces_host(faces)
        self.vmin = int(self.faces.max()) + 1                 # vertices the faces need
        self._adj = {}
        self._dev = {}

    def on(self, device, V: int):
        key = (str(device), V)
        if key not in self._dev:
            if V not in self._adj:
                self._adj[V] = face_adjacency(self.faces, V)
            start, face = self._adj[V]
            up = lambda a: torch.from_numpy(a).to(device)
            self._dev[key] = (up(self.faces), up(start), up(face if len(face) else np.zeros(1, np.int32)), len(face))
        return self._dev[key]


def _verts(lib, vertices, vmin: int):
    if not isinstance(vertices, torch.Tensor):
        raise ValueError('vertices must be a torch tensor on the device')
    _hip.check_device(lib, vertices)
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.dtype != torch.float32 or vertices.shape[0] < 1 or vertices.shape[1] < 1:
        raise ValueError(f'vertices must be float32 [B, V, 3], got {vertices.dtype} {tuple(vertices.shape)}')
    if vertices.shape[1] < vmin:
        raise ValueError(f'the faces name vertex {vmin - 1}, the mesh has {vertices.shape[1]} vertices')
    if vertices.shape[1] > 2 ** 24:
        raise ValueError('at most 2^24 vertices')
    return vertices.detach().contiguous()


def _normals_into(lib, verts, topo, normals, sums, chunk):
    B, V = verts.shape[:2]
    faces, start, face, nnz = topo.on(verts.device, V)
    s = lib.stream(verts.device)
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        sub = lambda t: None if t is None else ptr(t[lo:hi])
        lib.check(lib.vertex_normals(ptr(verts[lo:hi]), hi - lo, V, ptr(faces), faces.shape[0], ptr(start), ptr(face), nnz, sub(normals),
                                     sub(sums), s), 'vertex_normals')


def vertex_normals(vertices: torch.Tensor, faces, return_sums: bool = False, _lib: Optional[_hip.HipLib] = None):
    """Unit vertex normals [B, V, 3] of ``vertices`` [B, V, 3] float32 under ``faces`` [F, 3] (rule 1 of the module docstring);
    ``return_sums`` adds the unnormalised, area-weighted sums.  ``faces`` may be a ``BodyRenderer``'s ``topology`` to reuse its
    adjacency."""
    lib = _lib or _hip.get_lib()
    topo = faces if isinstance(faces, _Topology) else _Topology(faces)
    verts = _verts(lib, vertices, topo.vmin)
    normals = torch.empty_like(verts)
    sums = torch.empty_like(verts) if return_sums else None
    _normals_into(lib, verts, topo, normals, sums, MAX_FRAMES)
    return (normals, sums) if return_sums else normals


def _unit(v, what):
    v = float(v)
    if not (np.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError(f'{what} must be in [0, 1], got {v}')
    return v


class BodyRenderer:
    """Shaded overlays of a body mesh in a pinhole camera view.  ``faces`` [F, 3]; the camera defaults to PROX's render camera
    (``occlusion.PROX_RENDER``, fit_temp_loadprox_slide.py:626-640), ``cull_backface`` as in ``occlusion.py`` (an assumption about
    pyrender, both settings supported).  ``base_color``, ``ambient``, ``diffuse`` in [0, 1]: rule 3 of the module docstring.
    ``chunk`` frames go into one set of launches; any number of frames can be passed."""

    def __init__(self, faces, W: int = PROX_RENDER['W'], H: int = PROX_RENDER['H'], fx: float = PROX_RENDER['fx'],
                 fy: float = PROX_RENDER['fy'], cx: float = PROX_RENDER['cx'], cy: float = PROX_RENDER['cy'], znear: float = 0.05,
                 zfar: float = 100.0, cull_backface: bool = True, base_color=(1.0, 1.0, 0.9), ambient: float = 0.3, diffuse: float = 0.7,
                 chunk: int = 16, _lib: Optional[_hip.HipLib] = None):
        self.lib = _lib or _hip.get_lib()
        if not 1 <= int(chunk) <= MAX_FRAMES:
            raise ValueError(f'chunk must be 1 .. {MAX_FRAMES} frames')
        self.chunk = int(chunk)
        self._cam = _cam(W, H, fx, fy, cx, cy, znear, zfar, cull_backface)
        base = tuple(base_color) if np.ndim(base_color) == 1 else ()
        if len(base) != 3:
            raise ValueError('base_color must be three values in [0, 1]')
        self._shade = _hip.RenderShade((C.c_float * 3)(*[_unit(v, 'base_color') for v in base]), _unit(ambient, 'ambient'),
                                       _unit(diffuse, 'diffuse'))
        self.topology = _Topology(faces)
        self.W, self.H = self._cam.W, self._cam.H

    def _background(self, background, B, dev):
        if background is None:
            return None, 0, 0
        if not isinstance(background, torch.Tensor):
            raise ValueError('background must be a torch tensor on the device')
        _hip.check_device(self.lib, background)
        shape = tuple(background.shape)
        if background.dtype not in (torch.uint8, torch.float32) or shape not in ((self.H, self.W, 3), (B, self.H, self.W, 3)):
            raise ValueError(f'background must be uint8 or float32 [{self.H}, {self.W}, 3] or [{B}, {self.H}, {self.W}, 3], got '
                             f'{background.dtype} {shape}')
        if background.device != dev:
            raise ValueError('background and vertices are on different devices')
        return background.contiguous(), (1 if background.dtype == torch.uint8 else 2), int(background.dim() == 3)

    def _points(self, points, point_radius, point_color, B, dev):
        if points is None:
            return None, 0, 0
        if not isinstance(points, torch.Tensor):
            raise ValueError('points must be a torch tensor on the device')
        _hip.check_device(self.lib, points)
        if points.dim() != 3 or points.shape[-1] != 2 or points.dtype != torch.float32 or points.shape[0] != B or not 1 <= points.shape[1] <= 2 ** 20:
            raise ValueError(f'points must be float32 [B = {B}, P, 2] pixel coordinates, got {points.dtype} {tuple(points.shape)}')
        if points.device != dev:
            raise ValueError('points and vertices are on different devices')
        if int(point_radius) != point_radius or not 0 <= int(point_radius) <= MAX_RADIUS:
            raise ValueError(f'point_radius must be an integer 0 .. {MAX_RADIUS}, got {point_radius}')
        col = tuple(point_color) if np.ndim(point_color) == 1 else ()
        if len(col) != 3 or any(int(v) != v or not 0 <= int(v) <= 255 for v in col):
            raise ValueError('point_color must be three integers 0 .. 255')
        return points.detach().contiguous(), int(point_radius), (int(col[0]) << 16) | (int(col[1]) << 8) | int(col[2])

    def __call__(self, vertices: torch.Tensor, background: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None,
                 point_radius: int = 2, point_color=(255, 0, 0), return_depth: bool = False, return_face_ids: bool = False,
                 return_shade: bool = False):
        """vertices [B, V, 3] float32 in camera coordinates -> uint8 [B, H, W, 3]; ``background``: None, or uint8 / float32 in [0, 1]
        of [B, H, W, 3] or [H, W, 3] (shared by all frames, never copied); ``points`` [B, P, 2] float32 pixel coordinates drawn as
        discs of ``point_radius`` in ``point_color`` over the body.  Optional further outputs, in this order: depth float32 [B, H, W]
        (0: not covered), face ids int32 [B, H, W] (-1: not covered), shade float32 [B, H, W] (0: not covered)."""
        lib, topo = self.lib, self.topology
        verts = _verts(lib, vertices, topo.vmin)
        B, V = verts.shape[:2]
        dev = verts.device
        bg, bg_kind, bg_shared = self._background(background, B, dev)
        pts, radius, color = self._points(points, point_radius, point_color, B, dev)
        H, W, n = self.H, self.W, min(B, self.chunk)
        faces = topo.on(dev, V)[0]
        img = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        depth = torch.empty(B, H, W, dtype=torch.float32, device=dev) if return_depth else None
        fids = torch.empty(B, H, W, dtype=torch.int32, device=dev) if return_face_ids else None
        shade = torch.empty(B, H, W, dtype=torch.float32, device=dev) if return_shade else None
        keys = torch.empty(n, H, W, dtype=torch.int32, device=dev)
        ids = torch.empty(n, H, W, dtype=torch.int32, device=dev)
        normals = torch.empty(n, V, 3, dtype=torch.float32, device=dev)
        s = lib.stream(dev)
        cam = C.byref(self._cam)
        for lo in range(0, B, self.chunk):
            hi = min(B, lo + self.chunk)
            sub = lambda t: None if t is None else ptr(t[lo:hi])
            _normals_into(lib, verts[lo:hi], topo, normals, None, self.chunk)
            lib.check(lib.render_ids(ptr(verts[lo:hi]), hi - lo, V, ptr(faces), faces.shape[0], cam, ptr(keys), ptr(ids), sub(depth), s),
                      'render_ids')
            lib.check(lib.render_resolve(ptr(verts[lo:hi]), ptr(normals), hi - lo, V, ptr(faces), faces.shape[0], cam, ptr(ids),
                                         C.byref(self._shade), ptr(bg) if bg_shared else sub(bg), bg_kind, bg_shared, sub(img), sub(fids),
                                         sub(shade), s), 'render_resolve')
        if pts is not None:
            for lo in range(0, B, MAX_FRAMES):
                hi = min(B, lo + MAX_FRAMES)
                lib.check(lib.render_points(ptr(pts[lo:hi]), hi - lo, pts.shape[1], radius, W, H, color, ptr(img[lo:hi]), s), 'render_points')
        extra = tuple(t for t in (depth, fids, shade) if t is not None)
        return (img,) + extra if extra else img
