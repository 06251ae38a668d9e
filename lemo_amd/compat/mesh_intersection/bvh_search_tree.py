"""``BVH(max_collisions)``: ``triangles`` [B, F, 3, 3] -> int64 [B, C, 2] colliding triangle pairs, ``-1`` behind the last.

``C = min(F * max_collisions, MAX_PAIRS)``: the package sizes its output as ``F * max_collisions`` (2.7 million rows at the PROX
shape, nearly all ``-1``); the list here is compact, so 65536 rows hold every pair of a body mesh, and the first ``C`` in
lexicographic order are kept beyond that.  The corners of ``triangles`` carry no vertex index, so two triangles count as sharing a
vertex where two of their corners have equal coordinates in frame 0 (one ``torch.unique`` per call, which waits for the device: new
code should call ``lemo_amd.selfpen.find_collisions`` with the mesh's faces instead)."""
import torch

MAX_PAIRS = 1 << 16


def _check(triangles):
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 4 or tuple(triangles.shape[2:]) != (3, 3) or triangles.dtype != torch.float32:
        raise ValueError('triangles must be a float32 tensor [B, F, 3, 3]')
    return triangles.shape[0], triangles.shape[1]


class BVH(torch.nn.Module):
    def __init__(self, max_collisions=8):
        super().__init__()
        self.max_collisions = int(max_collisions)
        if self.max_collisions < 1:
            raise ValueError('max_collisions must be at least 1')

    @torch.no_grad()
    def forward(self, triangles):
        from . import _get_lib
        from ...selfpen import find_collisions
        B, F = _check(triangles)
        verts = triangles.detach().reshape(B, 3 * F, 3).contiguous()
        uniq, inverse = torch.unique(verts[0], dim=0, return_inverse=True)
        faces = inverse.reshape(F, 3).to(torch.int32)
        merged = verts.new_empty(B, uniq.shape[0], 3)
        merged[:, inverse] = verts                                  # corners that coincide in frame 0 are one vertex in every frame
        pairs = find_collisions(merged, faces, max_pairs=min(F * self.max_collisions, MAX_PAIRS), _lib=_get_lib())
        return pairs.long()
