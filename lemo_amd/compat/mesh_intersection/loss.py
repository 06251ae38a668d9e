"""``DistanceFieldPenetrationLoss(sigma, point2plane=False, vectorized=True, penalize_outside=True)``: ``(triangles [B, F, 3, 3],
collision_idxs [B, C, 2])`` -> [B], differentiable in ``triangles`` (``lemo_amd.selfpen.penetration_loss``)."""
import torch


class DistanceFieldPenetrationLoss(torch.nn.Module):
    def __init__(self, sigma=0.5, point2plane=False, vectorized=True, penalize_outside=True, linear_max=None):
        super().__init__()
        if point2plane or linear_max is not None:
            raise NotImplementedError('DistanceFieldPenetrationLoss: point2plane=True and linear_max are not provided')
        self.sigma, self.penalize_outside = float(sigma), bool(penalize_outside)

    def forward(self, triangles, collision_idxs):
        from . import _get_lib
        from .bvh_search_tree import _check
        from ...selfpen import penetration_loss
        B, F = _check(triangles)
        verts = triangles.reshape(B, 3 * F, 3)
        faces = torch.arange(3 * F, dtype=torch.int32, device=triangles.device).reshape(F, 3)
        return penetration_loss(verts, faces, collision_idxs.to(torch.int32).contiguous(), None, self.sigma, self.penalize_outside, _lib=_get_lib())
