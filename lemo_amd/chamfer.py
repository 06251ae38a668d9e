"""Chamfer nearest neighbours on the device (``csrc/chamfer_kernels.hip``) and the PROX scene-contact term built on them.

``temp_prox/dist_chamfer.py`` wraps a CUDA extension named ``chamfer``; ``SMPLifyLoss`` reaches it with ``contact: True``
(fitting_temp_slide.py:743-753) and through the ``s2m`` / ``m2s`` terms (:657-667).  Here

    dist1, dist2, idx1, idx2 = chamfer_distance(xyz1, xyz2)                  # [B, N, 3] x [B, M, 3]; SQUARED distances, int32 indices
    dist1, _, idx1, _ = chamfer_distance(xyz1, scene[None], bidirectional=False)   # one target set [1, M, 3] for the whole batch
    loss = contact_term(vertices_world, contact_verts_ids, scene_v, weight)  # the three lines of :747-753, differentiable

``ChamferDist()(a, b)`` has the call shape of the reference's ``chamferDist``.  A shared target set is never repeated B times and
the reverse direction is computed only when asked for (the reference computes it and throws it away).  Ties go to the lowest index.
Points must be finite: that is not checked (a check would wait for the device); a NaN coordinate never wins a comparison, so the
query it belongs to reports ``inf`` and the first index.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import ptr

# sizes of csrc/chamfer_kernels.hip (lemo_chamfer_sizes reports the same four; tests/chamfer_common.py compares them)
QUERIES_PER_WORKGROUP = 1024          # 256 lanes x 4 queries in registers
LDS_CHUNK = 512                       # targets per LDS buffer
SPLIT_LENGTH = 1024                   # an automatic split of the target range never holds fewer targets: 2 x this is the first M that splits
SPLIT_TARGET_WORKGROUPS = 1024        # the target range is cut until the launch has this many workgroups (or SPLIT_LENGTH stops it)
SHARED, REVERSE = 1, 2                # LEMO_CHAMFER_SHARED, LEMO_CHAMFER_REVERSE
MAX_BATCH = 65535
MAX_POINTS = 1 << 30                  # B x N and B x M


def library_sizes(lib: Optional[_hip.HipLib] = None) -> Tuple[int, int, int, int]:
    """(queries per workgroup, LDS chunk, split length, workgroups wanted) as the loaded library was built"""
    out = (C.c_int * 4)()
    (lib or _hip.get_lib()).chamfer_sizes(out)
    return tuple(out)


def _validate(lib, xyz1, xyz2, bidirectional: bool):
    """-> (B, N, M, shared); every refusal happens here, before a launch"""
    for name, t in (('xyz1', xyz1), ('xyz2', xyz2)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name} must be a torch tensor on the device')
        _hip.check_device(lib, t)
        if t.dtype != torch.float32:
            raise ValueError(f'{name} must be float32, got {t.dtype}')
        if t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f'{name} must be [B, points, 3], got {tuple(t.shape)}')
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f'{name} needs at least one batch entry and one point, got {tuple(t.shape)}')
    if xyz1.device != xyz2.device:
        raise ValueError('xyz1 and xyz2 are on different devices')
    B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if xyz2.shape[0] not in (B, 1):
        raise ValueError(f'xyz2 has {xyz2.shape[0]} batch entries, xyz1 has {B} (1 = one target set shared by all)')
    shared = xyz2.shape[0] == 1 and B > 1
    if shared and bidirectional:
        raise ValueError('the reverse direction is not defined for a shared target set [1, M, 3]: pass bidirectional=False')
    if B > MAX_BATCH or B * N > MAX_POINTS or B * M > MAX_POINTS:
        raise ValueError(f'at most {MAX_BATCH} batch entries and {MAX_POINTS} points per side, got B = {B}, N = {N}, M = {M}')
    return B, N, M, shared


def _forward(lib, xyz1, xyz2, bidirectional: bool, split: int = 0, out=None):
    """validated launch; ``out`` = (dist1, dist2, idx1, idx2) to fill in place (the compat entry), else fresh tensors"""
    B, N, M, shared = _validate(lib, xyz1, xyz2, bidirectional)
    split = int(split)
    if split < 0:
        raise ValueError(f'split must be 0 (automatic) or a positive count, got {split}')
    xyz1, xyz2 = xyz1.detach().contiguous(), xyz2.detach().contiguous()
    dev = xyz1.device
    flags = (SHARED if shared else 0) | (REVERSE if bidirectional else 0)
    if out is None:
        dist1 = torch.empty(B, N, dtype=torch.float32, device=dev)
        idx1 = torch.empty(B, N, dtype=torch.int32, device=dev)
        dist2 = torch.empty(B, M, dtype=torch.float32, device=dev) if bidirectional else None
        idx2 = torch.empty(B, M, dtype=torch.int32, device=dev) if bidirectional else None
    else:
        dist1, dist2, idx1, idx2 = out
    nbytes = int(lib.chamfer_workspace_bytes(B, N, M, flags, split))
    if nbytes < 0:
        raise ValueError(f'chamfer: shapes B = {B}, N = {N}, M = {M} are not taken')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    lib.check(lib.chamfer_forward(ptr(xyz1), ptr(xyz2), B, N, M, flags, split, ptr(dist1), ptr(idx1),
                                  None if dist2 is None else ptr(dist2), None if idx2 is None else ptr(idx2),
                                  None if ws is None else ptr(ws), nbytes, lib.stream(dev)), 'chamfer_forward')
    return dist1, dist2, idx1, idx2, (xyz1, xyz2, flags)


def _backward(lib, xyz1, xyz2, flags: int, g1, idx1, g2, idx2, need1: bool, need2: bool, out=None):
    """-> (grad1 or None, grad2 or None); a side that is not needed is neither computed nor written"""
    B, N, M = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if out is None:
        grad1 = torch.empty_like(xyz1) if need1 else None
        grad2 = torch.empty_like(xyz2) if need2 else None
    else:
        grad1, grad2 = out
    if grad1 is None and grad2 is None:
        return None, None
    rev = bool(flags & REVERSE)
    lib.check(lib.chamfer_backward(ptr(xyz1), ptr(xyz2), B, N, M, flags, ptr(g1), ptr(idx1), ptr(g2) if rev else None,
                                   ptr(idx2) if rev else None, None if grad1 is None else ptr(grad1),
                                   None if grad2 is None else ptr(grad2), lib.stream(xyz1.device)), 'chamfer_backward')
    return grad1, grad2


class _ChamferFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, bidirectional, split, lib):
        dist1, dist2, idx1, idx2, (x1, x2, flags) = _forward(lib, xyz1, xyz2, bidirectional, split)
        ctx.lib, ctx.flags, ctx.bidirectional = lib, flags, bidirectional
        if bidirectional:
            ctx.save_for_backward(x1, x2, idx1, idx2)
            ctx.mark_non_differentiable(idx1, idx2)
            return dist1, dist2, idx1, idx2
        ctx.save_for_backward(x1, x2, idx1)
        ctx.mark_non_differentiable(idx1)
        return dist1, idx1

    @staticmethod
    def backward(ctx, *grads):
        if ctx.bidirectional:
            x1, x2, idx1, idx2 = ctx.saved_tensors
            g1, g2 = grads[0].contiguous(), grads[1].contiguous()
        else:
            (x1, x2, idx1), idx2 = ctx.saved_tensors, None
            g1, g2 = grads[0].contiguous(), None
        grad1, grad2 = _backward(ctx.lib, x1, x2, ctx.flags, g1, idx1, g2, idx2, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return grad1, grad2, None, None, None


def chamfer_distance(xyz1: torch.Tensor, xyz2: torch.Tensor, bidirectional: bool = True, split: int = 0,
                     _lib: Optional[_hip.HipLib] = None):
    """``xyz1`` [B, N, 3], ``xyz2`` [B, M, 3] or [1, M, 3] (float32, on the device, finite) -> ``(dist1, dist2, idx1, idx2)``:
    ``dist1`` [B, N] the squared distance of every point of ``xyz1`` to a nearest point of ``xyz2`` and ``idx1`` its int32 index
    (lowest index on ties); ``dist2`` / ``idx2`` [B, M] the other way round, ``None`` with ``bidirectional=False``.  A shared target
    ``[1, M, 3]`` against B > 1 needs ``bidirectional=False``.  Differentiable with respect to both point sets (the indices are
    constants, as in the extension).  ``split`` (0 = automatic) cuts the target range into that many pieces; results do not depend
    on it.  Bad arguments raise ``ValueError`` before anything is launched; tensors off the device are refused (no CPU path)."""
    lib = _lib or _hip.get_lib()
    bidirectional = bool(bidirectional)
    if bidirectional:
        return _ChamferFunction.apply(xyz1, xyz2, True, split, lib)
    dist1, idx1 = _ChamferFunction.apply(xyz1, xyz2, False, split, lib)
    return dist1, None, idx1, None


class ChamferDist(torch.nn.Module):
    """``chamferDist`` of temp_prox/dist_chamfer.py:48-53: ``forward(input1, input2) -> (dist1, dist2, idx1, idx2)``"""

    def __init__(self, _lib: Optional[_hip.HipLib] = None):
        super().__init__()
        self._lib = _lib

    def forward(self, input1: torch.Tensor, input2: torch.Tensor):
        return chamfer_distance(input1, input2, True, _lib=self._lib)


def contact_ids_tensor(contact_verts_ids, V: int, device) -> torch.Tensor:
    """the contact vertex ids (LEMO's ``body_segments/*.json`` in the order of fit_temp_loadprox_slide.py:357-362; the caller's data)
    as an int64 index tensor, checked against the mesh once"""
    ids = contact_verts_ids.detach().cpu().numpy() if isinstance(contact_verts_ids, torch.Tensor) else np.asarray(contact_verts_ids)
    if ids.dtype.kind not in 'iu' or ids.ndim != 1 or ids.size < 1:
        raise ValueError(f'contact_verts_ids must be a non-empty 1-D list of integers, got {ids.dtype} {ids.shape}')
    if ids.min() < 0 or ids.max() >= V:
        raise ValueError(f'contact_verts_ids name vertices {int(ids.min())} .. {int(ids.max())}, the body has {V}')
    return torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(device)


def contact_term(vertices_world: torch.Tensor, contact_verts_ids, scene_v: torch.Tensor, weight,
                 _lib: Optional[_hip.HipLib] = None) -> torch.Tensor:
    """The body-scene contact energy of ``SMPLifyLoss`` (fitting_temp_slide.py:743-753):

        d = squared distance of vertices_world[:, contact_verts_ids] to the nearest scene vertex;  s = sqrt(d + 1e-4)
        weight * mean(s / (s + 1))

    ``vertices_world`` [B, V, 3]; ``scene_v`` [M, 3] or [1, M, 3] on the same device (a constant: it gets no gradient);
    ``contact_verts_ids``: integers, or an int64 tensor already on the device (``contact_ids_tensor``).  One-sided and shared: the
    scene is neither repeated per frame nor searched in the reverse direction."""
    if not isinstance(vertices_world, torch.Tensor) or vertices_world.dim() != 3 or vertices_world.shape[-1] != 3:
        raise ValueError('vertices_world must be a [B, V, 3] tensor')
    if not isinstance(scene_v, torch.Tensor) or scene_v.dim() not in (2, 3) or scene_v.shape[-1] != 3 or \
            (scene_v.dim() == 3 and scene_v.shape[0] != 1):
        raise ValueError('scene_v must be a [M, 3] or [1, M, 3] tensor')
    if isinstance(contact_verts_ids, torch.Tensor) and contact_verts_ids.dtype == torch.int64 and \
            contact_verts_ids.device == vertices_world.device and contact_verts_ids.dim() == 1:
        ids = contact_verts_ids
    else:
        ids = contact_ids_tensor(contact_verts_ids, vertices_world.shape[1], vertices_world.device)
    scene = scene_v.detach().reshape(1, -1, 3) if scene_v.dim() == 2 else scene_v.detach()
    body = vertices_world[:, ids, :].contiguous()
    d, _, _, _ = chamfer_distance(body, scene, bidirectional=False, _lib=_lib)
    s = torch.sqrt(d + 1e-4)
    return weight * (s / (s + 1.0)).mean()
