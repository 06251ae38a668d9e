"""``FilterFaces(faces_segm, faces_parents, ign_part_pairs)``: drops from an existing list [B, C, 2] the pairs whose faces lie in the
same part, in a part and its parent, or in an ignored pair of parts.  The survivors keep their order and move to the front, ``-1``
behind them.  Torch operations on the list's device; ``lemo_amd.selfpen.find_collisions`` applies the same rules inside the search."""
import numpy as np
import torch


class FilterFaces(torch.nn.Module):
    def __init__(self, faces_segm=None, faces_parents=None, ign_part_pairs=None):
        super().__init__()
        from ...selfpen import ign_table
        segm, par = np.asarray(faces_segm, np.int64), np.asarray(faces_parents, np.int64)
        if segm.ndim != 1 or par.shape != segm.shape:
            raise ValueError('faces_segm and faces_parents must be integers [F]')
        parts = int(max(segm.max(), par.max(), 0)) + 1
        self.register_buffer('faces_segm', torch.from_numpy(segm))
        self.register_buffer('faces_parents', torch.from_numpy(par))
        self.register_buffer('ign', torch.from_numpy(ign_table(ign_part_pairs, max(parts, 64)).astype(bool)))

    @torch.no_grad()
    def forward(self, collision_idxs):
        c = collision_idxs
        valid = (c[..., 0] >= 0) & (c[..., 1] >= 0)
        i, j = c[..., 0].clamp(min=0).long(), c[..., 1].clamp(min=0).long()
        si, sj, pi, pj = self.faces_segm[i], self.faces_segm[j], self.faces_parents[i], self.faces_parents[j]
        n = self.ign.shape[0]
        inside = (si >= 0) & (si < n) & (sj >= 0) & (sj < n)
        a, b = si.clamp(0, n - 1), sj.clamp(0, n - 1)
        drop = (si == sj) | (pi == sj) | (pj == si) | (inside & (self.ign[a, b] | self.ign[b, a]))
        keep = valid & ~drop
        order = torch.argsort((~keep).to(torch.int8), dim=-1, stable=True)
        out = torch.where(keep[..., None], c, torch.full_like(c, -1))
        return torch.gather(out, -2, order[..., None].expand_as(out))
