"""Time per call of the PROX depth terms (lemo_amd/scan.py: csrc/visibility_kernels.hip, lemo_chamfer_masked_forward).

    python tools/scan_terms_rate.py [--frames 100] [--out profiles/scan_terms_rate.txt]

Shape: B = 100 frames of the synthetic body model (V = 10475, 20908 faces from ``synthetic.local_faces`` over the posed vertices), a padded scan of S = 20000 points per frame
with 12000 .. 20000 valid ones, drawn from the camera-facing vertices plus 1 cm of noise.  Reported: vertex visibility in brute-force
and in binned mode (and the number of triangles the binned path tests against every vertex), the two masked searches, and the whole
``scan_terms`` forward + backward; next to them a torch baseline on the same device for the two searches: per-frame boolean
compaction, then chunked ``torch.cdist`` + ``min`` (forward only).  Device events, median and spread (min .. max) of 7 runs after 2
warm-up runs; each timed window repeats the call until it is >= 20 ms.  There is no earlier figure to compare with: the file
records what was measured and on which GPU.  ``auto`` in ``vertex_visibility`` means the faster of the two modes in THIS file.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd.scan import masked_nearest, scan_terms, vertex_visibility      # noqa: E402


def timed(fn, runs=7, warm=2, window_ms=20.0):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    reps = max(1, int(np.ceil(window_ms / max(a.elapsed_time(b), 1e-3))))
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def torch_baseline(q, t, qmask, tmask, chunk=4096):
    """per-frame boolean compaction, then chunked cdist + min"""
    outs = []
    for b in range(q.shape[0]):
        qq, tt = q[b][qmask[b]], t[b][tmask[b]]
        for lo in range(0, qq.shape[0], chunk):
            outs.append(torch.cdist(qq[lo:lo + chunk][None], tt[None]).min(2).values)
    return outs


def body_frames(B, device):
    import __graft_entry__ as G
    prob = G.prox_small_problem(B=B, V=10475)
    fit = G.prox_fitter_for(prob, device)[0]
    with torch.no_grad():
        body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(B, -1)
        verts = fit.body_model(return_verts=True, body_pose=body_pose).vertices.detach().contiguous()
    from lemo_amd import synthetic
    faces = synthetic.local_faces(verts[0].cpu().numpy(), 20908)      # the synthetic model's own faces are random triples, not a surface
    # local_faces triangulates ONE point cloud; the synthetic sequence's other poses would stretch those triangles across the body,
    # which no real body mesh does.  The frames are therefore rigid moves of frame 0: a turn about the vertical axis through its
    # centroid and a shift of a few centimetres per frame.
    v0 = verts[0].double()
    cen = v0.mean(0, keepdim=True)
    out = []
    for b in range(B):
        ang, c, s_ = 0.03 * b, np.cos(0.03 * b), np.sin(0.03 * b)
        R = torch.tensor([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]], dtype=torch.float64, device=device)
        out.append((v0 - cen) @ R.T + cen + torch.tensor([0.004 * b, 0.0, 0.003 * b], dtype=torch.float64, device=device))
    verts = torch.stack(out).float().contiguous()
    return verts, torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--scan', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'scan_terms_rate.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    B, S = a.frames, a.scan
    verts, faces = body_frames(B, dev)
    V, F = verts.shape[1], faces.shape[0]
    g = torch.Generator().manual_seed(0)
    vis_b = vertex_visibility(verts, faces, mode='brute')
    vis_g, nbig = vertex_visibility(verts, faces, mode='binned', return_big=True)
    same = bool(torch.equal(vis_b, vis_g))
    spn = torch.randint(12000 * S // 20000, S + 1, (B,), generator=g).to(torch.int32).to(dev)
    scan = torch.zeros(B, S, 3, device=dev)
    for b in range(B):
        ids = torch.nonzero(vis_b[b]).flatten()
        pick = ids[torch.randint(0, ids.numel(), (S,), generator=g).to(dev)]
        scan[b] = verts[b, pick] + 0.01 * torch.randn(S, 3, generator=g).to(dev)
        scan[b, int(spn[b]):] = 0.0
    body_mask = (torch.rand(V, generator=g) < 0.52).to(dev)
    valid = torch.arange(S, device=dev)[None] < spn[:, None]
    qm = vis_b.bool() & body_mask[None]
    lines = [f'scan_terms_rate: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'B = {B} frames, V = {V}, F = {F}, S = {S} padded scan points with {int(spn.min())} .. {int(spn.max())} valid; depth '
             f'{float(verts[..., 2].min()):.2f} .. {float(verts[..., 2].max()):.2f} m; visible share {float(vis_b.float().mean()):.3f}',
             f'brute force == binned on every bit: {same}; triangles per frame tested against every vertex (big or thin): median '
             f'{int(nbig.median())}, max {int(nbig.max())} of {F}',
             'ms per call: median (min .. max) of 7 runs']
    res = {}

    def row(name, fn):
        res[name] = timed(fn)
        lines.append(f'  {name:<58s} {res[name][0]:9.3f}  ({res[name][1]:.3f} .. {res[name][2]:.3f})')

    row('vertex_visibility brute', lambda: vertex_visibility(verts, faces, mode='brute'))
    row('vertex_visibility binned (grid 64)', lambda: vertex_visibility(verts, faces, mode='binned'))
    row('vertex_visibility binned (grid 32)', lambda: vertex_visibility(verts, faces, mode='binned', grid=32))
    row('masked_nearest s2m: scan -> visible vertices', lambda: masked_nearest(scan, verts, n1=spn, t_mask=vis_b))
    row('masked_nearest m2s: visible body vertices -> scan', lambda: masked_nearest(verts, scan, q_mask=qm, n2=spn))
    row('torch s2m: compaction + chunked cdist + min', lambda: torch_baseline(scan, verts, valid, vis_b.bool()))
    row('torch m2s: compaction + chunked cdist + min', lambda: torch_baseline(verts, scan, qm, valid))

    def whole():
        v = verts.clone().requires_grad_(True)
        s2m, m2s = scan_terms(v, faces, scan, spn, body_mask, 1.0, 1.0, 0.1, 0.1, check_counts=False)
        (s2m + m2s).backward()
    row('scan_terms forward + backward (auto visibility)', whole)
    fast = 'binned' if res['vertex_visibility binned (grid 64)'][0] < res['vertex_visibility brute'][0] else 'brute'
    lines.append(f'faster visibility mode at this shape in this run: {fast} '
                 f'(brute / binned = {res["vertex_visibility brute"][0] / res["vertex_visibility binned (grid 64)"][0]:.1f} x)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
