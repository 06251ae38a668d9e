"""The self-penetration term of ``SMPLifyLoss`` on the device (fitting_temp_slide.py:618-635; ``csrc/selfpen_kernels.hip``): what the
reference takes from the ``mesh_intersection`` package (torch-mesh-isect) -- the BVH collision search, ``FilterFaces`` and
``DistanceFieldPenetrationLoss`` -- for B frames at once.

    pairs, count = find_collisions(vertices, faces, faces_segm, faces_parents, ign, return_count=True)   # int32 [B, C, 2], int32 [B]
    L = penetration_loss(vertices, faces, pairs, count, sigma=1e-4)                                       # [B], differentiable
    term = self_penetration_term(vertices, faces, weight=w, faces_segm=..., faces_parents=..., ign_part_pairs=...)

What is restated rather than run: ``mesh_intersection`` is not part of this project's environment.  The definitions (the kernel
file's header states them in full) follow the published cone distance field (Tzionas et al., IJCV 2016, as used by SMPLify-X) and the
package's documented interface; conformance to the package bit for bit, or to the ulp, is NOT verified.  Triangles ``i < j`` collide
iff they share no vertex index, an edge of one meets the other (Moeller-Trumbore, inclusive; coplanar and degenerate triangles never
collide) and the part segmentation does not exclude the pair.  Everything takes and returns device tensors; there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _hip
from ._hip import ptr
from .scan import _faces, _points

MODES = {'auto': 0, 'brute': 1, 'grid': 2}             # LEMO_SELFPEN_AUTO, LEMO_SELFPEN_BRUTE, LEMO_SELFPEN_GRID
MAX_GRID = 16
MAX_PARTS = 64
DEFAULT_MAX_PAIRS = 16384


def ign_table(ign_part_pairs: Optional[Sequence[str]], parts: int = MAX_PARTS) -> np.ndarray:
    """``["9,16", "9,17", ...]`` (the YAML's ``ign_part_pairs``) -> uint8 [parts, parts] with 1 at ``[a, b]``; the search reads both
    ``[a, b]`` and ``[b, a]``"""
    t = np.zeros((parts, parts), np.uint8)
    for s in ign_part_pairs or ():
        ab = [int(x) for x in s.split(',')] if isinstance(s, str) else [int(x) for x in s]
        if len(ab) != 2 or min(ab) < 0 or max(ab) >= parts:
            raise ValueError(f'ign_part_pairs: {s!r} is not a pair of parts in 0 .. {parts - 1}')
        t[ab[0], ab[1]] = 1
    return t


def segmentation_from_weights(lbs_weights, faces, parents):
    """Stand-in for the licensed ``smplx_parts_segm.pkl``: a face's part is the arg-max skinning joint of its FIRST vertex, its parent
    that joint's kinematic parent -> ``(segm int32 [F], parents int32 [F])``.  Owners of the real file pass its ``segm`` / ``parents``."""
    w, f, p = np.asarray(lbs_weights), np.asarray(faces), np.asarray(parents).astype(np.int64)
    if w.ndim != 2 or f.ndim != 2 or f.shape[1] != 3 or p.shape != (w.shape[1],) or f.min() < 0 or f.max() >= w.shape[0]:
        raise ValueError(f'segmentation_from_weights: lbs_weights [V, J], faces [F, 3] inside the mesh, parents [J]; got {w.shape}, {f.shape}, {p.shape}')
    segm = np.argmax(w[f[:, 0]], axis=1).astype(np.int32)
    return segm, p[segm].astype(np.int32)


def _per_face(lib, a, F: int, device, name: str):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        _hip.check_device(lib, a)
        if a.dtype != torch.int32 or tuple(a.shape) != (F,) or a.device != device:
            raise ValueError(f'a {name} tensor must be int32 [{F}] on the vertices\' device, got {a.dtype} {tuple(a.shape)}')
        return a.contiguous()
    x = np.asarray(a)
    if x.dtype.kind not in 'iu' or x.shape != (F,):
        raise ValueError(f'{name} must be integers [{F}], got {x.dtype} {x.shape}')
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(device)


def _ign(lib, ign, device):
    """None, a list of "a,b" strings, or a uint8 / bool square table (numpy or device tensor) -> (uint8 [P, P] on the device, P)"""
    if ign is None:
        return None, 0
    if isinstance(ign, torch.Tensor):
        _hip.check_device(lib, ign)
        if ign.dtype not in (torch.uint8, torch.bool) or ign.dim() != 2 or ign.shape[0] != ign.shape[1] or not 1 <= ign.shape[0] <= MAX_PARTS \
                or ign.device != device:
            raise ValueError(f'an ign_part_pairs tensor must be uint8 / bool [P, P], P <= {MAX_PARTS}, on the vertices\' device')
        t = ign.contiguous()
        return (t.view(torch.uint8) if t.dtype == torch.bool else t), int(t.shape[0])
    if isinstance(ign, np.ndarray) and ign.ndim == 2:
        if ign.shape[0] != ign.shape[1] or not 1 <= ign.shape[0] <= MAX_PARTS or ign.dtype.kind not in 'biu':
            raise ValueError(f'an ign_part_pairs table must be square with at most {MAX_PARTS} parts, got {ign.dtype} {ign.shape}')
        t = (ign != 0).astype(np.uint8)
    else:
        t = ign_table(list(ign))
    return torch.from_numpy(np.ascontiguousarray(t)).to(device), int(t.shape[0])


def find_collisions(vertices: torch.Tensor, faces, faces_segm=None, faces_parents=None, ign_part_pairs=None,
                    max_pairs: int = DEFAULT_MAX_PAIRS, mode: str = 'auto', grid: int = 0, return_count: bool = False,
                    _lib: Optional[_hip.HipLib] = None):
    """``vertices`` [B, V, 3] float32 on the device, ``faces`` [F, 3] (numpy, or int32 on the device) -> int32 [B, max_pairs, 2]: the
    colliding triangle pairs ``(i, j)``, ``i < j``, of every frame in lexicographic order, ``-1`` behind the last; when a frame has more
    than ``max_pairs`` the first ``max_pairs`` in that order are kept.  ``return_count`` adds int32 [B]: the true number per frame.
    ``faces_segm`` / ``faces_parents`` (integers [F]) and ``ign_part_pairs`` (``["9,16", ...]`` or a square table) drop the pairs
    ``FilterFaces`` drops: same part, a part and its parent, an ignored pair of parts.  Detached (the list is a constant of the
    iteration, as in the reference), deterministic, no host synchronisation.  ``mode``: 'brute' tests every pair behind a box reject;
    'grid' bins the faces of each frame into a ``grid``^3 lattice (0 = 16); 'auto' is the faster at the PROX shape
    (profiles/selfpen_rate.txt).  The answer does not depend on ``mode`` or ``grid``, bit for bit."""
    lib = _lib or _hip.get_lib()
    _points(lib, vertices, 'vertices')
    if mode not in MODES:
        raise ValueError(f'mode must be one of {sorted(MODES)}, got {mode!r}')
    grid, C = int(grid), int(max_pairs)
    if grid < 0 or grid == 1 or grid > MAX_GRID:
        raise ValueError(f'grid must be 0 (default) or 2 .. {MAX_GRID}, got {grid}')
    if C < 1:
        raise ValueError(f'max_pairs must be at least 1, got {max_pairs}')
    B, V, dev = vertices.shape[0], vertices.shape[1], vertices.device
    f = _faces(lib, faces, V, dev)
    F = f.shape[0]
    if (faces_parents is not None or ign_part_pairs is not None) and faces_segm is None:
        raise ValueError('faces_parents / ign_part_pairs need faces_segm')
    segm, par = _per_face(lib, faces_segm, F, dev, 'faces_segm'), _per_face(lib, faces_parents, F, dev, 'faces_parents')
    ign, P = _ign(lib, ign_part_pairs, dev)
    v = vertices.detach().contiguous()
    nbytes = int(lib.selfpen_search_workspace_bytes(B, V, F, MODES[mode], grid))
    if nbytes < 0 or B * C > (1 << 28):
        raise ValueError(f'find_collisions: shapes B = {B}, V = {V}, F = {F}, max_pairs = {C} are not taken')
    pairs = torch.empty(B, C, 2, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib.check(lib.selfpen_search(ptr(v), B, V, ptr(f), F, ptr(segm), ptr(par), ptr(ign), P, MODES[mode], grid, ptr(pairs), C, ptr(count),
                                 ptr(ws), nbytes, lib.stream(dev)), 'selfpen_search')
    return (pairs, count) if return_count else pairs


class _PenetrationLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, f, pairs, count, sigma, outside, lib):
        v = vertices.detach().contiguous()
        B, V, dev = v.shape[0], v.shape[1], v.device
        L = torch.empty(B, dtype=torch.float32, device=dev)
        lib.check(lib.selfpen_loss_forward(ptr(v), B, V, ptr(f), f.shape[0], ptr(pairs), pairs.shape[1], ptr(count), sigma, outside, ptr(L),
                                           lib.stream(dev)), 'selfpen_loss_forward')
        ctx.lib, ctx.sigma, ctx.outside = lib, sigma, outside
        ctx.count = count
        ctx.save_for_backward(v, f, pairs)
        return L

    @staticmethod
    def backward(ctx, g):
        v, f, pairs = ctx.saved_tensors
        lib, B, V = ctx.lib, v.shape[0], v.shape[1]
        gv = torch.empty_like(v)
        g = g.detach().to(torch.float32).contiguous()
        lib.check(lib.selfpen_loss_backward(ptr(v), B, V, ptr(f), f.shape[0], ptr(pairs), pairs.shape[1], ptr(ctx.count), ctx.sigma, ctx.outside,
                                            ptr(g), ptr(gv), lib.stream(v.device)), 'selfpen_loss_backward')
        return gv, None, None, None, None, None, None


def _sigma(sigma) -> float:
    if isinstance(sigma, torch.Tensor) or not np.isfinite(float(sigma)) or float(sigma) <= 0:
        raise ValueError(f'sigma must be a finite host number > 0, got {sigma!r}')
    return float(sigma)


def penetration_loss(vertices: torch.Tensor, faces, pairs: torch.Tensor, count: Optional[torch.Tensor], sigma: float,
                     penalize_outside: bool = True, point2plane: bool = False, linear_max=None,
                     _lib: Optional[_hip.HipLib] = None) -> torch.Tensor:
    """``DistanceFieldPenetrationLoss(sigma, point2plane=False, vectorized=True, penalize_outside)`` -> [B]: for every listed pair the
    cone distance field of each triangle at the other's three corners, squared and summed (the module docstring's definition).
    ``pairs`` int32 [B, C, 2] and ``count`` int32 [B] (or None: all C entries, those that name no face are skipped) as
    ``find_collisions`` returns them.  Differentiable in ``vertices``: through the corners and through the normal, circumcentre and
    circumradius of the receiving triangle.  A zero-area triangle contributes nothing; an empty list gives 0 and a zero gradient
    without a look at the list on the host.  ``point2plane=True`` and ``linear_max`` are not provided."""
    if point2plane or linear_max is not None:
        raise NotImplementedError('penetration_loss: point2plane=True and linear_max are not provided')
    lib = _lib or _hip.get_lib()
    _points(lib, vertices, 'vertices')
    B, V, dev = vertices.shape[0], vertices.shape[1], vertices.device
    f = _faces(lib, faces, V, dev)
    if not isinstance(pairs, torch.Tensor):
        raise ValueError('pairs must be an int32 tensor [B, C, 2] on the device')
    _hip.check_device(lib, pairs)
    if pairs.dtype != torch.int32 or pairs.dim() != 3 or pairs.shape[0] != B or pairs.shape[1] < 1 or pairs.shape[2] != 2 or pairs.device != dev \
            or B * pairs.shape[1] > (1 << 28):
        raise ValueError(f'pairs must be int32 [B = {B}, C, 2] on the vertices\' device, got {pairs.dtype} {tuple(pairs.shape)}')
    if count is not None:
        if not isinstance(count, torch.Tensor):
            raise ValueError('count must be an int32 tensor [B] on the device, or None')
        _hip.check_device(lib, count)
        if count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != dev:
            raise ValueError(f'count must be int32 [{B}] on the vertices\' device, got {count.dtype} {tuple(count.shape)}')
        count = count.contiguous()
    return _PenetrationLoss.apply(vertices, f, pairs.contiguous(), count, _sigma(sigma), int(bool(penalize_outside)), lib)


def self_penetration_term(vertices: torch.Tensor, faces, weight, faces_segm=None, faces_parents=None, ign_part_pairs=None,
                          sigma: float = 1e-4, penalize_outside: bool = True, max_pairs: int = DEFAULT_MAX_PAIRS, mode: str = 'auto',
                          _lib: Optional[_hip.HipLib] = None) -> torch.Tensor:
    """fitting_temp_slide.py:618-635: ``sum(weight * L)`` with the collision search on the detached vertices.  The reference's
    ``collision_idxs.ge(0).sum().item() > 0`` is not needed: an empty list gives an exact 0 on the device.  ``weight``: a host number
    >= 0; 0 launches nothing."""
    if isinstance(weight, torch.Tensor) or not np.isfinite(float(weight)) or float(weight) < 0:
        raise ValueError(f'weight must be a finite number >= 0 (a host number: a zero weight launches nothing), got {weight!r}')
    sigma = _sigma(sigma)
    if not weight > 0:
        lib = _lib or _hip.get_lib()
        _points(lib, vertices, 'vertices')
        return torch.zeros((), dtype=torch.float32, device=vertices.device)
    pairs, count = find_collisions(vertices, faces, faces_segm, faces_parents, ign_part_pairs, max_pairs=max_pairs, mode=mode, return_count=True,
                                   _lib=_lib)
    return torch.sum(weight * penetration_loss(vertices, faces, pairs, count, sigma, penalize_outside, _lib=_lib))
