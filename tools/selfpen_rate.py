"""Rate of the self-penetration term (lemo_amd.selfpen, csrc/selfpen_kernels.hip) at the PROX shape: B = 100 frames, V = 10475,
F = 20908.  Input: the posed synthetic body (coherent skinning, a surface-sized mesh over the posed cloud) with the arms pushed into
the torso by a frame-dependent amount.  Measures the collision search (brute force / grid sizes / auto), the loss forward and the loss
forward + backward, next to the same loss composed in torch on the same pair list.  Writes profiles/selfpen_rate.txt; the grid / brute
line is what SP_AUTO_MODE in the kernel file is set from.

    python tools/selfpen_rate.py [--frames 100] [--reps 10] [--out profiles/selfpen_rate.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARM_JOINTS = (16, 17, 18, 19, 20, 21)
TORSO_JOINTS = (3, 6, 9)


def body(B, device):
    """-> (verts float32 [B, V, 3] on the device, faces int64 [F, 3], segm, parents)"""
    import __graft_entry__ as G
    from lemo_amd import synthetic
    from lemo_amd.selfpen import segmentation_from_weights
    prob = G.prox_small_problem(B=2, V=10475, coherent=True)
    fit = G.prox_fitter_for(prob, device)[0]
    with torch.no_grad():
        pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(2, -1)
        v0 = fit.body_model(return_verts=True, body_pose=pose).vertices[0].detach().cpu().numpy().astype(np.float64)
    faces = synthetic.local_faces(v0, 20908)
    dom = np.argmax(prob['model']['weights'], axis=1)
    arms, torso = np.isin(dom, ARM_JOINTS), np.isin(dom, TORSO_JOINTS)
    shift = v0[torso].mean(0) - v0[arms].mean(0)
    frames = []
    for b in range(B):
        v = v0.copy()
        v[arms] += shift * (0.55 + 0.4 * b / max(B - 1, 1))
        frames.append(v + np.array([0.003 * b, -0.002 * b, 0.004 * b]))
    par = np.where(synthetic.SMPLX_PARENTS < 0, -1, synthetic.SMPLX_PARENTS)
    segm, parents = segmentation_from_weights(prob['model']['weights'], faces, par)
    return torch.from_numpy(np.stack(frames).astype(np.float32)).to(device), faces, segm, parents


def torch_loss(verts, faces_t, pairs, count, sigma):
    """the definition composed in torch (float32) on the same list, every frame at once; masked where the kernel skips"""
    B, C = pairs.shape[0], pairs.shape[1]
    live = (torch.arange(C, device=verts.device)[None, :] < count[:, None]) & (pairs[..., 0] >= 0)
    idx = pairs.clamp(min=0).long()
    tri = verts[:, faces_t]                                           # [B, F, 3, 3]
    bi = torch.arange(B, device=verts.device)[:, None]
    total = 0
    for r, p in ((0, 1), (1, 0)):
        R, P = tri[bi, idx[..., r]], tri[bi, idx[..., p]]              # [B, C, 3, 3]
        p0, p1, p2 = R[..., 0, :], R[..., 1, :], R[..., 2, :]
        N = torch.linalg.cross(p1 - p0, p2 - p0)
        A2 = N.norm(dim=-1)
        ok = live & (A2 > 0)
        A2s = torch.where(ok, A2, torch.ones_like(A2))
        n = N / A2s[..., None]
        a2, b2, c2 = ((p1 - p2) ** 2).sum(-1), ((p2 - p0) ** 2).sum(-1), ((p0 - p1) ** 2).sum(-1)
        w1, w2 = b2 * (c2 + a2 - b2), c2 * (a2 + b2 - c2)
        ws = torch.where(ok, a2 * (b2 + c2 - a2) + w1 + w2, torch.ones_like(a2))
        o = p0 + (w1[..., None] * (p1 - p0) + w2[..., None] * (p2 - p0)) / ws[..., None]
        rad = torch.sqrt(a2 * b2 * c2 + (~ok).float()) / (2 * A2s)
        d = P - o[..., None, :]
        h = (d * n[..., None, :]).sum(-1)
        q = d - h[..., None] * n[..., None, :]
        rho = torch.sqrt((q * q).sum(-1) + 1e-30)
        D = rad[..., None] - (rad[..., None] / sigma) * h
        phi = rho / torch.where(D > 0, D, torch.ones_like(D))
        k2, k1 = (1 - 2 * sigma) / (4 * sigma * sigma), 1 / (2 * sigma)
        ups = torch.where(h <= -sigma, -h + 1 - sigma, torch.where(h < sigma, -k2 * h * h - k1 * h + (3 - 2 * sigma) / 4, torch.zeros_like(h)))
        psi = torch.where((D > 0) & (phi < 1) & ok[..., None], (1 - phi) * ups, torch.zeros_like(ups))
        total = total + (psi ** 2).sum((-1, -2))
    return total


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'selfpen_rate.txt'))
    a = ap.parse_args()
    from lemo_amd.selfpen import find_collisions, penetration_loss
    device = torch.device('cuda', 0)
    verts, faces, segm, parents = body(a.frames, device)
    B, V, F, C, sigma = verts.shape[0], verts.shape[1], len(faces), 1 << 16, 1e-4
    ft = torch.from_numpy(faces.astype(np.int32)).to(device)
    lines = [f'self-penetration term, B = {B}, V = {V}, F = {F}, capacity {C}, sigma {sigma}; {torch.cuda.get_device_name(0)}; median (min) of {a.reps} runs, ms']
    pairs, count = find_collisions(verts, ft, max_pairs=C, mode='brute', return_count=True)
    n = count.cpu().numpy()
    lines.append(f'colliding pairs per frame: min {n.min()}, median {int(np.median(n))}, max {n.max()} (unfiltered)')
    for name, kw in (('brute', dict(mode='brute')), ('grid 16', dict(mode='grid', grid=16)), ('grid 8', dict(mode='grid', grid=8)), ('auto', dict(mode='auto'))):
        got = find_collisions(verts, ft, max_pairs=C, return_count=True, **kw)
        assert torch.equal(got[0], pairs) and torch.equal(got[1], count), name
        med, mn = timed(lambda: find_collisions(verts, ft, max_pairs=C, **kw), a.reps)
        lines.append(f'search {name:8s} {med:9.3f} ({mn:.3f})')
    sg = torch.from_numpy(segm).to(device), torch.from_numpy(parents).to(device)
    med, mn = timed(lambda: find_collisions(verts, ft, sg[0], sg[1], max_pairs=C), a.reps)
    lines.append(f'search auto + part filter {med:9.3f} ({mn:.3f})')
    med, mn = timed(lambda: penetration_loss(verts, ft, pairs, count, sigma), a.reps)
    lines.append(f'loss forward              {med:9.3f} ({mn:.3f})')

    def fb(fn):
        v = verts.clone().requires_grad_(True)
        fn(v).sum().backward()
        return v.grad
    med, mn = timed(lambda: fb(lambda v: penetration_loss(v, ft, pairs, count, sigma)), a.reps)
    lines.append(f'loss forward + backward   {med:9.3f} ({mn:.3f})')
    Ct = int(min(C, max(int(n.max()), 1)))
    pt = pairs[:, :Ct].contiguous()
    ftl = ft.long()
    L = penetration_loss(verts, ft, pairs, count, sigma)
    Lt = torch_loss(verts, ftl, pt, count, sigma)
    lines.append(f'torch composition on the same list (first {Ct} columns): largest relative difference of L {float(((L - Lt).abs() / L.clamp(min=1e-30)).max()):.2e}')
    med, mn = timed(lambda: torch_loss(verts, ftl, pt, count, sigma), a.reps)
    lines.append(f'torch forward             {med:9.3f} ({mn:.3f})')
    med, mn = timed(lambda: fb(lambda v: torch_loss(v, ftl, pt, count, sigma)), a.reps)
    lines.append(f'torch forward + backward  {med:9.3f} ({mn:.3f})')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
