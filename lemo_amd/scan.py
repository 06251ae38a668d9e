"""The PROX depth terms on the device: body-vertex visibility (``csrc/visibility_kernels.hip``), nearest neighbours between point sets
whose valid part differs per frame (``lemo_chamfer_masked_forward`` in ``csrc/chamfer_kernels.hip``), and the scan-to-mesh /
mesh-to-scan energies of ``SMPLifyLoss`` built on them (fitting_temp_slide.py:637-670, ``s2m: True`` / ``m2s: True``).

    vis = vertex_visibility(vertices, faces)                                  # uint8 [B, V], 1 = the camera sees the vertex
    dist, idx = masked_nearest(scan, vertices, n1=scan_point_num, t_mask=vis) # squared distances, per-frame valid sets
    s2m, m2s = scan_terms(vertices, faces, scan, scan_point_num, body_mask, s2m_weight, m2s_weight)

What is restated rather than run: ``psbody.mesh`` is not part of this project's environment, so ``vertex_visibility`` follows what
``visibility_compute(v, f, cams)`` does on paper with its default ``min_dist = 1e-3`` and no normals or sensors -- vertex at p,
camera at c: the vertex is visible iff the segment from ``p + min_dist (c - p) / |c - p|`` to c meets no triangle of the mesh,
triangles at the vertex included, from either side; degenerate triangles never hit; ``|c - p| <= min_dist`` is visible.  This
definition is recalled from psbody's source, NOT confirmed by a run.  ``min_dist`` is a parameter.  Everything takes and returns
device tensors; there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import ptr
from .chamfer import MAX_BATCH, MAX_POINTS, _backward

MODES = {'auto': 0, 'brute': 1, 'binned': 2}          # LEMO_VIS_AUTO, LEMO_VIS_BRUTE, LEMO_VIS_BINNED
MAX_GRID = 64


def _faces(lib, faces, V: int, device) -> torch.Tensor:
    """int32 [F, 3] on the device.  A numpy array / list is checked against the mesh here; a device tensor is taken as it is (a check
    would wait for the device; the kernels skip a face that names a missing vertex)."""
    if isinstance(faces, torch.Tensor):
        _hip.check_device(lib, faces)
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError(f'a faces tensor must be int32 [F, 3], got {faces.dtype} {tuple(faces.shape)}')
        if faces.device != device:
            raise ValueError('faces and vertices are on different devices')
        return faces.contiguous()
    f = np.asarray(faces)
    if f.dtype.kind not in 'iu' or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f'faces must be integers [F, 3], got {f.dtype} {f.shape}')
    if f.min() < 0 or f.max() >= V:
        raise ValueError(f'faces name vertices {int(f.min())} .. {int(f.max())}, the mesh has {V}')
    return torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(device)


def _points(lib, t, name: str):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{name} must be a torch tensor on the device')
    _hip.check_device(lib, t)
    if t.dtype != torch.float32:
        raise ValueError(f'{name} must be float32, got {t.dtype}')
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f'{name} must be [B, points, 3] with at least one entry and one point, got {tuple(t.shape)}')
    if t.shape[0] > MAX_BATCH or t.shape[0] * t.shape[1] > MAX_POINTS:
        raise ValueError(f'{name}: at most {MAX_BATCH} batch entries and {MAX_POINTS} points, got {tuple(t.shape)}')


def _cam(lib, cam, B: int, device) -> Optional[torch.Tensor]:
    """None (the origin) or float32 [B, 3] on the device; a [3] position is shared by the frames"""
    if cam is None:
        return None
    if not isinstance(cam, torch.Tensor):
        c = np.asarray(cam, np.float32)
        if c.shape not in ((3,), (B, 3)) or not np.all(np.isfinite(c)):
            raise ValueError(f'cam must be a finite [3] or [B, 3] position, got {c.shape}')
        cam = torch.from_numpy(np.broadcast_to(c, (B, 3)).copy()).to(device)
    else:
        _hip.check_device(lib, cam)
        if cam.dtype != torch.float32 or tuple(cam.shape) not in ((3,), (B, 3)) or cam.device != device:
            raise ValueError(f'a cam tensor must be float32 [3] or [B, 3] on the vertices\' device, got {cam.dtype} {tuple(cam.shape)}')
        cam = cam.detach().expand(B, 3).contiguous()
    return cam


def vertex_visibility(vertices: torch.Tensor, faces, cam=None, min_dist: float = 1e-3, mode: str = 'auto', grid: int = 0,
                      return_big: bool = False, _lib: Optional[_hip.HipLib] = None):
    """``vertices`` [B, V, 3] float32 on the device, ``faces`` [F, 3] (numpy, or int32 on the device), ``cam``: the camera position
    ([3] or [B, 3]; None = the origin, PROX's camera coordinates) -> uint8 [B, V], 1 = visible (see the module docstring for the
    definition).  Detached: visibility is a constant of the iteration, as in the reference.  ``mode``: 'brute' tests every (vertex,
    triangle) pair; 'binned' bins the projected vertices into a ``grid`` x ``grid`` raster per frame (0 = 64) and lets every triangle
    visit the cells under its projection -- a frame with a vertex at or behind the camera plane takes the brute-force path by itself;
    'auto' is the faster of the two at the PROX shape (profiles/scan_terms_rate.txt).  The answer does not depend on ``mode`` or
    ``grid``, bit for bit.  ``return_big`` adds int32 [B]: the triangles of each frame that were tested against every vertex."""
    lib = _lib or _hip.get_lib()
    _points(lib, vertices, 'vertices')
    if mode not in MODES:
        raise ValueError(f'mode must be one of {sorted(MODES)}, got {mode!r}')
    grid, min_dist = int(grid), float(min_dist)
    if grid < 0 or grid == 1 or grid > MAX_GRID:
        raise ValueError(f'grid must be 0 (default) or 2 .. {MAX_GRID}, got {grid}')
    if not np.isfinite(min_dist) or min_dist < 0:
        raise ValueError(f'min_dist must be finite and not negative, got {min_dist}')
    B, V = vertices.shape[0], vertices.shape[1]
    dev = vertices.device
    f = _faces(lib, faces, V, dev)
    c = _cam(lib, cam, B, dev)
    v = vertices.detach().contiguous()
    nbytes = int(lib.vertex_visibility_workspace_bytes(B, V, f.shape[0], MODES[mode], grid))
    if nbytes < 0:
        raise ValueError(f'vertex_visibility: shapes B = {B}, V = {V}, F = {f.shape[0]} are not taken')
    vis = torch.empty(B, V, dtype=torch.uint8, device=dev)
    nbig = torch.empty(B, dtype=torch.int32, device=dev) if return_big else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    lib.check(lib.vertex_visibility(ptr(v), B, V, ptr(f), f.shape[0], ptr(c), min_dist, MODES[mode], grid, ptr(vis), ptr(nbig), ptr(ws),
                                    nbytes, lib.stream(dev)), 'vertex_visibility')
    return (vis, nbig) if return_big else vis


def _count(lib, n, B: int, limit: int, device, name: str):
    if n is None:
        return None
    if not isinstance(n, torch.Tensor):
        raise ValueError(f'{name} must be an int32 tensor [B] on the device (nothing off the device is taken)')
    _hip.check_device(lib, n)
    if n.dtype != torch.int32 or tuple(n.shape) != (B,) or n.device != device:
        raise ValueError(f'{name} must be int32 [{B}] on the points\' device, got {n.dtype} {tuple(n.shape)}')
    return n.contiguous()


def _mask(lib, m, B: int, P: int, device, name: str):
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise ValueError(f'{name} must be a uint8 / bool tensor [B, points] on the device')
    _hip.check_device(lib, m)
    if m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (B, P) or m.device != device:
        raise ValueError(f'{name} must be uint8 or bool [{B}, {P}] on the points\' device, got {m.dtype} {tuple(m.shape)}')
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


class _MaskedNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, n1, q_mask, n2, t_mask, split, lib):
        B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        x1, x2 = xyz1.detach().contiguous(), xyz2.detach().contiguous()
        dev = x1.device
        dist = torch.empty(B, N, dtype=torch.float32, device=dev)
        idx = torch.empty(B, N, dtype=torch.int32, device=dev)
        nbytes = int(lib.chamfer_workspace_bytes(B, N, M, 0, split))
        if nbytes < 0:
            raise ValueError(f'masked_nearest: shapes B = {B}, N = {N}, M = {M} are not taken')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        lib.check(lib.chamfer_masked_forward(ptr(x1), ptr(x2), B, N, M, ptr(n1), ptr(q_mask), ptr(n2), ptr(t_mask), split, ptr(dist),
                                             ptr(idx), ptr(ws), nbytes, lib.stream(dev)), 'chamfer_masked_forward')
        ctx.lib = lib
        ctx.save_for_backward(x1, x2, idx)
        ctx.mark_non_differentiable(idx)
        return dist, idx

    @staticmethod
    def backward(ctx, g, _gi):
        x1, x2, idx = ctx.saved_tensors
        # lemo_chamfer_backward, unchanged, flags = 0: idx = -1 (an invalid query, an entry without a valid target) gets no gradient
        grad1, grad2 = _backward(ctx.lib, x1, x2, 0, g.contiguous(), idx, None, None, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return grad1, grad2, None, None, None, None, None, None


def masked_nearest(xyz1: torch.Tensor, xyz2: torch.Tensor, n1=None, q_mask=None, n2=None, t_mask=None, split: int = 0,
                   _lib: Optional[_hip.HipLib] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``xyz1`` [B, N, 3] queries, ``xyz2`` [B, M, 3] targets (float32, on the device, finite) -> ``(dist1, idx1)`` [B, N]: the
    squared distance to, and the int32 index of, the nearest VALID target.  Query i of entry b is valid iff ``i < n1[b]`` (``n1``
    int32 [B] on the device, or None = all) and ``q_mask[b, i]`` (uint8 / bool [B, N], or None); targets likewise with ``n2`` /
    ``t_mask``; a count and a mask given together both have to hold.  Indices refer to the original arrays, lowest index on ties.
    An invalid query, and every query of an entry without a valid target, reports ``dist = 0`` and ``idx = -1`` and takes part in no
    gradient.  Differentiable in both point sets.  With everything valid the result equals ``chamfer_distance(...,
    bidirectional=False)`` bit for bit; it never depends on ``split``.  The masks are read where they are: nothing is compacted and
    nothing waits for the device.  Bad arguments raise ``ValueError`` before anything is launched."""
    lib = _lib or _hip.get_lib()
    _points(lib, xyz1, 'xyz1')
    _points(lib, xyz2, 'xyz2')
    if xyz1.device != xyz2.device:
        raise ValueError('xyz1 and xyz2 are on different devices')
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError(f'xyz1 has {xyz1.shape[0]} batch entries, xyz2 has {xyz2.shape[0]}')
    split = int(split)
    if split < 0:
        raise ValueError(f'split must be 0 (automatic) or a positive count, got {split}')
    B, N, M, dev = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1], xyz1.device
    n1, n2 = _count(lib, n1, B, N, dev, 'n1'), _count(lib, n2, B, M, dev, 'n2')
    q_mask, t_mask = _mask(lib, q_mask, B, N, dev, 'q_mask'), _mask(lib, t_mask, B, M, dev, 't_mask')
    return _MaskedNearest.apply(xyz1, xyz2, n1, q_mask, n2, t_mask, split, lib)


def gmof(d_squared: torch.Tensor, rho) -> torch.Tensor:
    """Geman-McClure on the SQUARED distance: ``rho^2 d / (d + rho^2)``.  The reference's ``GMoF`` (misc_utils.py:69-72) is handed
    ``sqrt(d)`` and squares it again: the same value, but the root's gradient is NaN at ``d == 0`` (a scan point that coincides with a
    vertex).  This form has the finite gradient ``rho^4 / (d + rho^2)^2`` there."""
    r2 = rho * rho
    return r2 * d_squared / (d_squared + r2)


def scan_terms(vertices: torch.Tensor, faces, scan: torch.Tensor, scan_point_num: torch.Tensor, body_mask: torch.Tensor, s2m_weight,
               m2s_weight, rho_s2m=1.0, rho_m2s=1.0, cam=None, min_dist: float = 1e-3, check_counts: bool = True,
               _lib: Optional[_hip.HipLib] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The scan-to-mesh and mesh-to-scan energies of ``SMPLifyLoss`` (fitting_temp_slide.py:637-670) -> ``(s2m_dist, m2s_dist)``.

    ``vertices`` [B, V, 3] and ``scan`` [B, S, 3] in CAMERA coordinates (:644-667 use ``body_model_output.vertices`` before the
    cam-to-world step); ``scan_point_num`` int32 [B]: the leading valid points of each frame's padded scan; ``body_mask`` bool [V]:
    the vertices that take part in m2s (the complement of ``body_segments/body_mask.json``'s head ids, fit_temp_loadprox_slide.py:
    421-426); all on the device.  With vis = ``vertex_visibility(vertices, faces, cam, min_dist)``, for every frame that has at least
    one visible vertex and at least one scan point

        s2m_b = mean over the valid scan points of gmof(squared distance to the nearest VISIBLE vertex, rho_s2m)
        m2s_b = mean over the vertices with vis & body_mask of gmof(squared distance to the nearest valid scan point, rho_m2s)

    and each term is ``weight x mean of those frames`` (m2s also leaves out a frame without any vis & body_mask vertex, whose mean
    does not exist); 0 where there is no such frame or the weight is 0.  A term with weight 0 launches nothing, and with both at 0 not
    even the visibility runs.  Gradients flow to ``vertices`` (and ``scan``); visibility is a constant.

    Three differences to the reference, none reproduced: it computes both directions in both calls and throws one away (here each
    term runs one one-sided search); with only one of the two terms enabled it divides by the length of an empty list (:669-670
    raise ZeroDivisionError; here the other term is simply 0); and it skips frames with ``vis.sum() == 0`` by a host round trip (here
    such frames drop out of the means on the device).  The robustifier is ``gmof`` on the squared distance (see there).
    ``check_counts`` reads ``scan_point_num`` back once to refuse a count outside 0 .. S; pass False inside an optimisation loop
    whose counts were checked when they were loaded (the counts are then clamped on the device).
    The two searches and the visibility are HIP kernels; the elementwise GMoF and the per-frame means are torch operations."""
    lib = _lib or _hip.get_lib()
    _points(lib, vertices, 'vertices')
    _points(lib, scan, 'scan')
    B, V, S, dev = vertices.shape[0], vertices.shape[1], scan.shape[1], vertices.device
    if scan.shape[0] != B or scan.device != dev:
        raise ValueError(f'scan must be [B = {B}, S, 3] on the vertices\' device, got {tuple(scan.shape)} on {scan.device}')
    spn = _count(lib, scan_point_num, B, S, dev, 'scan_point_num')
    if spn is None:
        raise ValueError('scan_point_num must be an int32 tensor [B] on the device')
    if not isinstance(body_mask, torch.Tensor) or body_mask.dtype != torch.bool or tuple(body_mask.shape) != (V,) or body_mask.device != dev:
        raise ValueError(f'body_mask must be a bool tensor [{V}] on the vertices\' device')
    f = _faces(lib, faces, V, dev)
    c = _cam(lib, cam, B, dev)
    for name, w in (('s2m_weight', s2m_weight), ('m2s_weight', m2s_weight)):
        if isinstance(w, torch.Tensor) or not np.isfinite(float(w)) or float(w) < 0:
            raise ValueError(f'{name} must be a finite number >= 0 (a host number: a zero weight launches nothing), got {w!r}')
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    if not (s2m_weight > 0 or m2s_weight > 0):
        return zero, zero
    if check_counts and (int(spn.min()) < 0 or int(spn.max()) > S):   # the one read of device data; a caller that has checked its
        raise ValueError(f'scan_point_num must lie in 0 .. S = {S}')  # counts once (ProxTemporalFitter) passes check_counts=False
    spn = torch.clamp(spn, 0, S)
    vis = vertex_visibility(vertices, f, c, min_dist, _lib=lib)
    scan_valid = torch.arange(S, device=dev)[None, :] < spn[:, None]
    frame = (spn > 0) & (vis.sum(1) > 0)
    s2m, m2s = zero, zero
    if s2m_weight > 0:
        d, _ = masked_nearest(scan, vertices, n1=spn, t_mask=vis, _lib=lib)
        per = (gmof(d, rho_s2m) * scan_valid).sum(1) / spn.clamp(min=1)
        s2m = s2m_weight * (per * frame).sum() / frame.sum().clamp(min=1)
    if m2s_weight > 0:
        qm = vis.bool() & body_mask[None, :]
        d, _ = masked_nearest(vertices, scan, q_mask=qm, n2=spn, _lib=lib)
        cnt = qm.sum(1)
        per = (gmof(d, rho_m2s) * qm).sum(1) / cnt.clamp(min=1)
        fr = frame & (cnt > 0)
        m2s = m2s_weight * (per * fr).sum() / fr.sum().clamp(min=1)
    return s2m, m2s
