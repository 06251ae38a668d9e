"""Scene (SDF) terms of the PROX fitting loss on the HIP kernels.

Reference: temp_prox/fitting_temp_slide.py:685-739 -- ``F.grid_sample(self.sdf, norm_vertices[:, :, [2,1,0]]...,
padding_mode='border')`` on a 256^3 signed-distance volume.  The reference repeats the volume B times
(fit_temp_loadprox_slide.py:299, 6.7 GB at B = 100); here one copy is sampled by all frames.

``build_scene_sdf`` makes that volume from a scene mesh on the device (``csrc/scene_sdf_kernels.hip``, whose header states the
definition in full): the exact distance from every voxel centre to the nearest point of the mesh, negative behind the surface by the
angle-weighted pseudonormal of the closest feature.  PROX ships ``<scene>_sdf.npy`` for its twelve scenes and never published the
program that made them: the definition here is this project's, and whether PROX's generator sampled at the same voxel centres (the
points where ``sdf_sample`` has interpolation weight 0) is unknown.

    S = build_scene_sdf(vertices, faces, dim=256)             # SceneSdf: .sdf [D, H, W], .grid_min, .grid_max, .dims
    fit = ProxTemporalFitter(..., **S.fitter_kwargs(), ...)
    S.save_prox(sdf_dir, 'MyRoom'); S = load_prox_sdf(sdf_dir, 'MyRoom', device)
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _hip
from ._hip import ptr


class _SdfSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, sdf, gmin, gmax, lib):
        shape = pts.shape[:-1]
        p = pts.reshape(-1, 3).contiguous().float()
        _hip.check_device(lib, p)
        N = p.shape[0]
        val = torch.empty(N, dtype=torch.float32, device=p.device)
        dval = torch.empty(N, 3, dtype=torch.float32, device=p.device)
        D, H, W = sdf.shape
        g0 = (C.c_float * 3)(*[float(v) for v in gmin])
        g1 = (C.c_float * 3)(*[float(v) for v in gmax])
        lib.check(lib.sdf_sample(ptr(sdf), D, H, W, ptr(p), N, g0, g1, ptr(val), ptr(dval), lib.stream(p.device)), 'sdf_sample')
        ctx.save_for_backward(dval)
        ctx.shape = pts.shape
        return val.view(shape)

    @staticmethod
    def backward(ctx, g):
        (dval,) = ctx.saved_tensors
        return (dval * g.reshape(-1, 1)).view(ctx.shape), None, None, None, None


def sdf_sample(points_world: torch.Tensor, sdf: torch.Tensor, grid_min, grid_max, _lib=None) -> torch.Tensor:
    """points_world [...,3] -> sdf value [...]; sdf [D,H,W] float32 contiguous on the same device."""
    assert sdf.dim() == 3 and sdf.is_contiguous() and sdf.dtype == torch.float32
    return _SdfSample.apply(points_world, sdf, grid_min, grid_max, _lib or _hip.get_lib())


# ---------------------------------------------------------------------------------------------------------------- mesh -> SDF volume
SDF_MODES = {'auto': 0, 'brute': 1, 'grid': 2}          # LEMO_SCENE_SDF_AUTO, LEMO_SCENE_SDF_BRUTE, LEMO_SCENE_SDF_GRID
SDF_MAX_SIDE = 1024
SDF_MAX_VOXELS = 1 << 28
SDF_MAX_FACES = 1 << 22
SDF_MAX_VERTICES = 1 << 24
SDF_MAX_GRID = 32
SDF_LDS_CHUNK = 256                                     # triangles per LDS buffer of the kernels (tests straddle it)
SDF_BRICK = (4, 8, 8)                                   # voxels per workgroup


def mesh_normal_tables(vertices: np.ndarray, faces: np.ndarray):
    """The three tables of the sign rule, in float64 from the mesh alone -> (face_n [F, 3], edge_n [F, 3, 3], vert_n [V, 3], valid [F]).
    A face is valid iff its indices lie in [0, V), its corners are finite and its area is positive; an invalid face has a zero
    ``face_n`` (the kernels ignore it on that mark) and adds nothing to the other tables.  ``edge_n[f, e]``: edge e of face f is
    (v0 v1, v1 v2, v2 v0); the sum of the unit normals of all valid faces that share that undirected edge (adjacency by sorting the
    edge keys).  ``vert_n[v]``: the unit normals of the valid faces at v, weighted by their corner angles."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    V, F = v.shape[0], f.shape[0]
    inside = np.all((f >= 0) & (f < V), axis=1)
    fc = np.where(inside[:, None], f, 0)
    c = v[fc]                                                                            # [F, 3, 3]
    with np.errstate(all='ignore'):
        n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ln = np.sqrt(np.sum(n * n, axis=1))
        valid = inside & np.all(np.isfinite(c.reshape(F, 9)), axis=1) & np.isfinite(ln) & (ln > 0)
        unit = np.where(valid[:, None], n / np.where(valid, ln, 1.0)[:, None], 0.0)
        unit32 = unit.astype(np.float32)
        valid &= np.any(unit32 != 0, axis=1)                                             # the mark must survive the rounding
        unit = np.where(valid[:, None], unit, 0.0)
        # corner angles
        ang = np.zeros((F, 3))
        for k in range(3):
            e1, e2 = c[:, (k + 1) % 3] - c[:, k], c[:, (k + 2) % 3] - c[:, k]
            cr = np.sqrt(np.sum(np.cross(e1, e2) ** 2, axis=1))
            ang[:, k] = np.where(valid, np.arctan2(cr, np.sum(e1 * e2, axis=1)), 0.0)
    ang = np.nan_to_num(ang, nan=0.0, posinf=0.0, neginf=0.0)
    vert_n = np.zeros((V, 3))
    for a in range(3):
        vert_n[:, a] = np.bincount(fc.reshape(-1), weights=(ang * unit[:, None, a]).reshape(-1), minlength=V)
    # undirected edges: key = min * V + max, one sorted pass
    i0, i1 = fc, np.roll(fc, -1, axis=1)                                                 # edge e = (v_e, v_{e+1})
    key = (np.minimum(i0, i1) * V + np.maximum(i0, i1)).reshape(-1)
    _, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    per_edge = np.repeat(unit, 3, axis=0)                                                # [3F, 3], zero for invalid faces
    edge_n = np.zeros((3 * F, 3))
    for a in range(3):
        edge_n[:, a] = np.bincount(inv, weights=per_edge[:, a])[inv]
    edge_n = np.where(np.repeat(valid, 3)[:, None], edge_n, 0.0).reshape(F, 3, 3)
    return unit, edge_n, vert_n, valid


class SceneMesh(NamedTuple):
    """a scene mesh prepared for ``build_scene_sdf``: device tensors plus the bounding box of the valid triangles (host)"""
    vertices: torch.Tensor
    faces: torch.Tensor
    face_n: torch.Tensor
    edge_n: torch.Tensor
    vert_n: torch.Tensor
    box_min: Optional[np.ndarray]
    box_max: Optional[np.ndarray]


def prepare_scene_mesh(vertices: torch.Tensor, faces, _lib=None) -> SceneMesh:
    """Validate the mesh and build its normal tables once (host numpy in float64, one copy of the vertices to the host, rounded to
    fp32 and uploaded).  ``vertices`` float32 [V, 3] on the device; ``faces`` [F, 3]: a numpy array / list of integers inside the mesh,
    or an int32 device tensor (taken as it is: the kernels ignore a face that names a missing vertex)."""
    from .occlusion import _mesh
    lib = _lib or _hip.get_lib()
    v, f = _mesh(lib, vertices, faces, batched=False)
    if v.shape[0] > SDF_MAX_VERTICES or f.shape[0] > SDF_MAX_FACES:
        raise ValueError(f'build_scene_sdf takes at most {SDF_MAX_VERTICES} vertices and {SDF_MAX_FACES} faces, got {v.shape[0]} and {f.shape[0]}')
    v = v.detach()
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    face_n, edge_n, vert_n, valid = mesh_normal_tables(vh, fh)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(v.device)
    lo = hi = None
    if valid.any():
        used = vh[fh[valid].reshape(-1)].astype(np.float64)
        lo, hi = used.min(axis=0), used.max(axis=0)
    return SceneMesh(v, f, up(face_n), up(edge_n), up(vert_n), lo, hi)


def _bound(x, name):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, np.float64).reshape(-1)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f'{name} must be three finite numbers, got {x!r}')
    return a


class SceneSdf:
    """A signed-distance volume and its box.  ``sdf`` float32 [D, H, W] on the device, indexed [x, y, z]; ``grid_min`` / ``grid_max``
    float32 numpy [3]; ``dims`` = (D, H, W); ``nearest`` int32 [D, H, W] (the winning face per voxel, -1 without one) or None."""

    def __init__(self, sdf: torch.Tensor, grid_min, grid_max, nearest: Optional[torch.Tensor] = None):
        self.sdf, self.nearest = sdf, nearest
        self.grid_min, self.grid_max = np.asarray(grid_min, np.float32).copy(), np.asarray(grid_max, np.float32).copy()
        self.dims = tuple(int(d) for d in sdf.shape)

    def centres(self) -> torch.Tensor:
        """float32 [D, H, W, 3]: ``grid_min + (i + 0.5) * (grid_max - grid_min) / dim`` per axis, evaluated in float32 -- the points where
        ``sdf_sample`` has interpolation weight 0"""
        dev, ax = self.sdf.device, []
        for a in range(3):
            step = np.float32((self.grid_max[a] - self.grid_min[a]) / np.float32(self.dims[a]))
            ax.append((torch.arange(self.dims[a], dtype=torch.float32, device=dev) + 0.5) * float(step) + float(self.grid_min[a]))
        return torch.stack(torch.meshgrid(*ax, indexing='ij'), dim=-1)

    def fitter_kwargs(self) -> dict:
        """``dict(sdf=, grid_min=, grid_max=)`` for ``ProxTemporalFitter`` and the window engine"""
        return dict(sdf=self.sdf, grid_min=self.grid_min, grid_max=self.grid_max)

    def save_prox(self, sdf_dir: str, scene_name: str) -> None:
        """write ``<scene>.json`` (keys ``min``, ``max``, ``dim``) and ``<scene>_sdf.npy`` (dim^3 float32), exactly what
        fit_temp_loadprox_slide.py:287-294 reads.  That format holds one ``dim``: a volume that is not cubic raises ``ValueError``."""
        D, H, W = self.dims
        if not D == H == W:
            raise ValueError(f"PROX's sdf files hold one dim: the volume must be cubic, got {self.dims}")
        os.makedirs(sdf_dir, exist_ok=True)
        with open(os.path.join(sdf_dir, scene_name + '.json'), 'w') as fh:
            json.dump({'min': [float(x) for x in self.grid_min], 'max': [float(x) for x in self.grid_max], 'dim': D}, fh)
        np.save(os.path.join(sdf_dir, scene_name + '_sdf.npy'), self.sdf.detach().cpu().numpy().reshape(-1))


def load_prox_sdf(sdf_dir: str, scene_name: str, device) -> SceneSdf:
    """the inverse of ``SceneSdf.save_prox``; reads PROX's own files the way fit_temp_loadprox_slide.py:286-294 does"""
    with open(os.path.join(sdf_dir, scene_name + '.json')) as fh:
        meta = json.load(fh)
    dim = int(meta['dim'])
    vol = np.load(os.path.join(sdf_dir, scene_name + '_sdf.npy')).reshape(dim, dim, dim)
    sdf = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(device)
    return SceneSdf(sdf, np.array(meta['min'], np.float32), np.array(meta['max'], np.float32))


def build_scene_sdf(vertices, faces=None, dim=256, grid_min=None, grid_max=None, padding: float = 0.25, mode: str = 'auto',
                    grid: Optional[int] = None, return_nearest: bool = False, _lib=None) -> SceneSdf:
    """Scene mesh -> ``SceneSdf``: the signed-distance volume ``ProxTemporalFitter``, the native PROX engine and ``sdf_sample`` take.

    ``vertices`` float32 [V, 3] on the device in scene / world coordinates and ``faces`` [F, 3] (see ``prepare_scene_mesh``), or a
    ``SceneMesh`` from ``prepare_scene_mesh`` alone: its tables are reused, and with explicit bounds the call then touches the host
    nowhere (it can be captured in a graph).  ``dim``: an int or (D, H, W) = voxels along x, y, z.  Without explicit ``grid_min`` /
    ``grid_max`` the box is the bounding box of the valid triangles widened by ``padding`` metres on every side; 0.25 is this API's
    default, not a PROX value (PROX's boxes come with its files).  ``mode``: 'brute' streams every triangle past every voxel, 'grid'
    searches a ``grid``^3 cell grid outward from each brick of voxels (``grid`` None = max(dim) / 8 clamped to 2 .. 32), 'auto' is
    'grid' except for tiny meshes.  The volume does not depend on ``mode`` or ``grid``, bit for bit, and repeated runs are
    bit-identical.  ``return_nearest`` adds the winning face per voxel.  A mesh without a valid triangle gives +inf everywhere (and
    needs explicit bounds).  Limits: each side <= 1024, D H W <= 2^28, F <= 2^22, V <= 2^24.  There is no CPU path."""
    lib = _lib or _hip.get_lib()
    if isinstance(vertices, SceneMesh):
        if faces is not None:
            raise ValueError('a SceneMesh carries its faces')
        mesh = vertices
        _hip.check_device(lib, mesh.vertices)
    else:
        if faces is None:
            raise ValueError('faces are missing')
        mesh = None
    if mode not in SDF_MODES:
        raise ValueError(f'mode must be one of {sorted(SDF_MODES)}, got {mode!r}')
    g = 0 if grid is None else int(grid)
    if grid is not None and not 2 <= g <= SDF_MAX_GRID:
        raise ValueError(f'grid must be None or 2 .. {SDF_MAX_GRID}, got {grid!r}')
    dims = (dim,) * 3 if isinstance(dim, (int, np.integer)) else tuple(dim) if isinstance(dim, (tuple, list)) else ()
    if len(dims) != 3 or any(not isinstance(d, (int, np.integer)) or isinstance(d, bool) for d in dims):
        raise ValueError(f'dim must be an int or three ints, got {dim!r}')
    D, H, W = (int(d) for d in dims)
    if min(D, H, W) < 1 or max(D, H, W) > SDF_MAX_SIDE or D * H * W > SDF_MAX_VOXELS:
        raise ValueError(f'dim: each side in 1 .. {SDF_MAX_SIDE} and at most {SDF_MAX_VOXELS} voxels, got {(D, H, W)}')
    if (grid_min is None) != (grid_max is None):
        raise ValueError('grid_min and grid_max come together')
    if not np.isfinite(float(padding)) or float(padding) < 0:
        raise ValueError(f'padding must be a finite number >= 0, got {padding!r}')
    if grid_min is not None:
        lo, hi = _bound(grid_min, 'grid_min'), _bound(grid_max, 'grid_max')
    if mesh is None:
        mesh = prepare_scene_mesh(vertices, faces, _lib=lib)
    if grid_min is None:
        if mesh.box_min is None:
            raise ValueError('the mesh has no valid triangle: give grid_min and grid_max')
        lo, hi = mesh.box_min - float(padding), mesh.box_max + float(padding)
    with np.errstate(all='ignore'):
        lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
        ext = hi32 - lo32
    if not (np.all(np.isfinite(lo32)) and np.all(np.isfinite(hi32)) and np.all(np.isfinite(ext)) and np.all(ext > 0)):
        raise ValueError(f'the box {lo.tolist()} .. {hi.tolist()} is empty or not finite in float32')
    v, f = mesh.vertices, mesh.faces
    V, F, dev = v.shape[0], f.shape[0], v.device
    nbytes = int(lib.scene_sdf_ws_bytes(F, D, H, W, SDF_MODES[mode], g))
    if nbytes < 0:
        raise ValueError(f'build_scene_sdf: F = {F}, dim = {(D, H, W)} are not taken')
    sdf = torch.empty(D, H, W, dtype=torch.float32, device=dev)
    nearest = torch.empty(D, H, W, dtype=torch.int32, device=dev) if return_nearest else None
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    g0, g1 = (C.c_float * 3)(*[float(x) for x in lo32]), (C.c_float * 3)(*[float(x) for x in hi32])
    lib.check(lib.scene_sdf_build(ptr(v), V, ptr(f), F, ptr(mesh.face_n), ptr(mesh.edge_n), ptr(mesh.vert_n), g0, g1, D, H, W, SDF_MODES[mode], g,
                                  ptr(sdf), ptr(nearest), ptr(ws), nbytes, lib.stream(dev)), 'scene_sdf_build')
    return SceneSdf(sdf, lo32, hi32, nearest)
