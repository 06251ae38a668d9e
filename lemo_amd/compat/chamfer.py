"""Stand-in for the ``chamfer`` CUDA extension (temp_prox/dist_chamfer.py:27,43), served by ``csrc/chamfer_kernels.hip``.

LEMO's fitting configurations S2 / S3 set the Chamfer terms' weights to 0 and never reach it; ``contact: True``
(fitting_temp_slide.py:743-753) and the ``s2m`` / ``m2s`` terms do.  ``forward`` / ``backward`` fill the caller's tensors in place,
exactly as the extension does, so ``temp_prox/dist_chamfer.py`` runs unmodified on device tensors.  There is no CPU path: calling
either with anything that is not a device tensor is an error (``NotImplementedError``), not a silent fall-back.

New code should call ``lemo_amd.chamfer.chamfer_distance`` / ``contact_term``: they skip the reverse direction and share one
target set over the batch, which this call shape cannot express.
"""
import torch

_lib = None          # tests only: the host-emulated library (it takes CPU tensors and nothing else)


def _library(tensors, what):
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        raise NotImplementedError(f'chamfer.{what}: no CPU path -- every argument must be a tensor on the HIP device')
    on_device = (lambda t: not t.is_cuda) if _lib is not None and _lib.is_emu else (lambda t: t.is_cuda)
    if not all(on_device(t) for t in tensors):
        raise NotImplementedError(f'chamfer.{what}: no CPU path -- every argument must be a tensor on the HIP device')
    if _lib is not None:
        return _lib
    from .. import _hip
    return _hip.get_lib()


def _check(xyz1, xyz2, outs):
    """(B, N, M) of the extension's call: equal batch sizes, the caller's buffers in the wrapper's shapes and types"""
    from ..chamfer import _validate
    for t, shape, dtype in outs:
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != xyz1.device:
            raise ValueError(f'chamfer: expected a contiguous {dtype} buffer of shape {shape} on {xyz1.device}, '
                             f'got {t.dtype} {tuple(t.shape)} on {t.device}')


def forward(xyz1, xyz2, dist1, dist2, idx1, idx2):
    """dist1 [B, N], dist2 [B, M] (float32) and idx1, idx2 (int32) are overwritten with the squared nearest-neighbour distances and
    indices of xyz1 [B, N, 3] against xyz2 [B, M, 3] and back"""
    lib = _library((xyz1, xyz2, dist1, dist2, idx1, idx2), 'forward')
    from ..chamfer import _forward, _validate
    if xyz2.dim() == 3 and xyz1.dim() == 3 and xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError(f'chamfer.forward: batch sizes {xyz1.shape[0]} and {xyz2.shape[0]} differ')
    B, N, M, _ = _validate(lib, xyz1, xyz2, True)
    _check(xyz1, xyz2, ((dist1, (B, N), torch.float32), (dist2, (B, M), torch.float32), (idx1, (B, N), torch.int32),
                        (idx2, (B, M), torch.int32)))
    _forward(lib, xyz1, xyz2, True, out=(dist1, dist2, idx1, idx2))
    return 1


def backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
    """gradxyz1 [B, N, 3] and gradxyz2 [B, M, 3] are overwritten with the gradients for graddist1 [B, N], graddist2 [B, M]"""
    lib = _library((xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2), 'backward')
    from ..chamfer import REVERSE, _backward, _validate
    if xyz2.dim() == 3 and xyz1.dim() == 3 and xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError(f'chamfer.backward: batch sizes {xyz1.shape[0]} and {xyz2.shape[0]} differ')
    B, N, M, _ = _validate(lib, xyz1, xyz2, True)
    _check(xyz1, xyz2, ((gradxyz1, (B, N, 3), torch.float32), (gradxyz2, (B, M, 3), torch.float32), (graddist1, (B, N), torch.float32),
                        (graddist2, (B, M), torch.float32), (idx1, (B, N), torch.int32), (idx2, (B, M), torch.int32)))
    _backward(lib, xyz1.detach().contiguous(), xyz2.detach().contiguous(), REVERSE, graddist1, idx1, graddist2, idx2, True, True,
              out=(gradxyz1, gradxyz2))
    return 1
