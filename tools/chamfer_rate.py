"""Pair-evaluations per second of the Chamfer nearest-neighbour kernels (lemo_amd/chamfer.py, csrc/chamfer_kernels.hip).

    python tools/chamfer_rate.py [--scene 200000] [--out profiles/chamfer_rate.txt]

Two shapes: the PROX contact term (B = 100 frames x 1121 contact vertices against ONE shared scene, one-sided; the scene's
``--scene`` vertices are an ASSUMPTION, no PROX scene mesh is part of this project) and an ``s2m``-like call (B = 1, 20 000 scan
points against the 10 475 body vertices, both directions).  Each is timed forward and forward + backward, next to a chunked
``torch.cdist`` + ``min`` on the same device (forward only; for the shared scene it is given the scene once, not B copies).

Roof: the arithmetic is fp32 VALU work with no matrix-core form.  256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-operations/s
(half the 157.3 TFLOPS vector peak, which counts a fused multiply-add as two).  The kernel spends 9 lane-operations per pair
(3 subtractions, 1 multiply, 2 fused multiply-adds, 1 compare, 2 selects): 8.74 T pairs/s.  The reported fraction is of that figure.
Device events, median of 7 runs after 2 warm-up runs of the same shape; each timed window repeats the call until it is >= 20 ms.
There is no earlier figure to compare with: the file records what was measured and on which GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd.chamfer import chamfer_distance                    # noqa: E402

LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
OPS_PER_PAIR = 9
ROOF = LANE_OPS_PER_S / OPS_PER_PAIR


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
    return float(np.median(out)), out


def cdist_min(x1, x2, both, chunk=4096):
    """the torch formulation on the same device: all-pairs distances in row chunks, min + argmin (not squared, not tie-exact)"""
    B = x1.shape[0]
    t = x2.expand(B, -1, -1) if x2.shape[0] != B else x2
    outs = []
    for lo in range(0, x1.shape[1], chunk):
        outs.append(torch.cdist(x1[:, lo:lo + chunk], t).min(2))
    if both:
        for lo in range(0, t.shape[1], chunk):
            outs.append(torch.cdist(t[:, lo:lo + chunk], x1).min(2))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scene', type=int, default=200_000)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'chamfer_rate.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a rate is measured on the GPU'
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    shapes = [('contact term (scene size is an assumption)', 100, 1121, args.scene, False, True),
              ('s2m-like', 1, 20_000, 10_475, True, False)]
    lines = [f'{torch.cuda.get_device_name(0)}; device events, median of 7 runs after 2 warm-ups, windows >= 20 ms; '
             f'roof {ROOF / 1e12:.2f} T pairs/s = 78.6 T fp32 lane-operations/s / {OPS_PER_PAIR} per pair (VALU, no matrix-core form)']
    fmt = lambda rs: ', '.join(f'{v:.3f}' for v in rs)
    for name, B, N, M, both, shared in shapes:
        x1 = (torch.randn(B, N, 3, generator=g) * 0.5 + torch.tensor([3.0, 3.0, 1.0])).to(dev)
        x2 = (torch.rand(1 if shared else B, M, 3, generator=g) * torch.tensor([6.0, 6.0, 2.5])).to(dev)
        pairs = B * N * M * (2 if both else 1)
        ms_f, runs_f = timed(lambda: chamfer_distance(x1, x2, bidirectional=both))
        x1g = x1.clone().requires_grad_(True)
        x2g = x2.clone().requires_grad_(both)

        def fb():
            x1g.grad = None
            x2g.grad = None
            d1, d2, _, _ = chamfer_distance(x1g, x2g, bidirectional=both)
            (d1.sum() + (d2.sum() if both else 0.0)).backward()
        ms_fb, runs_fb = timed(fb)
        ms_t, runs_t = timed(lambda: cdist_min(x1, x2, both))
        lines += [f'{name}: B = {B}, N = {N}, M = {M}, {"both directions" if both else "one-sided"}, {"shared target" if shared else "per-entry targets"}; '
                  f'{pairs / 1e9:.2f} G pairs',
                  f'  forward            {ms_f:.3f} ms = {pairs / ms_f / 1e9:.3f} T pairs/s = {pairs / ms_f / 1e-3 / ROOF:.3f} of the VALU roof   (runs: {fmt(runs_f)})',
                  f'  forward + backward {ms_fb:.3f} ms (the backward touches {B * N * (2 if both else 1)} points, with the sum and autograd around it)   (runs: {fmt(runs_fb)})',
                  f'  torch.cdist + min, chunks of 4096 rows, forward only: {ms_t:.3f} ms = {pairs / ms_t / 1e9:.3f} T pairs/s   (runs: {fmt(runs_t)})']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
