"""Time per call of the VPoser encoder (lemo_amd/vposer.py ``VPoser.encode``: csrc/vposer_enc_kernels.hip), forward and forward + backward.

    python tools/vposer_encode_rate.py [--out profiles/vposer_encode_rate.txt]

Shapes: B = 119 (one fitting window; not the target) and B = 100 000 (a data set or every frame of a recording: the target).  Rows:
  lemo_vposer_encode_fwd / _bwd alone   the C entries with preallocated outputs: one launch each
  VPoser.encode                         the method (allocations, the autograd Function, the Normal object), no_grad / with backward of
                                        (mean * gm + std * gs).sum()
  nn modules, fp32                      the same layers as the class's own nn modules on the same device in float32: BatchNorm1d ->
                                        Linear -> leaky_relu -> BatchNorm1d -> Linear -> leaky_relu -> two Linear heads -> softplus,
                                        forward under no_grad and forward + autograd backward to the input
Device events on the current stream, median and spread (min .. max) of 7 runs after 2 warm-up calls; each timed window repeats the call
until it is >= 200 ms.  Next to the device-event time every row shows the host's time to ISSUE one call: where the two are equal the row
measures the host's enqueue rate, not the device.  FLOP/s: 2 x (64 x 512 + 512 x 512 + 512 x 64) = 655 360 FLOP per pose forward (the
same again backward) as counted from the shapes, over the launch's event time: for the 'alone' rows that is one kernel plus its launch
gap, so a lower bound of the kernel's share of the fp32 matrix peak (157.3 TFLOP/s).  A record, not a gate.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd import _hip                                                               # noqa: E402
from lemo_amd._hip import ptr                                                           # noqa: E402
from lemo_amd.vposer import VPoser, make_vposer_enc_weights, make_vposer_weights        # noqa: E402

FLOP_PER_POSE = 2 * (64 * 512 + 512 * 512 + 512 * 64)
PEAK = 157.3e12


def timed(fn, runs=7, warm=2, window_ms=200.0):
    """-> (median, min, max) ms per call by device events, and the median host time to issue one call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    reps = max(1, int(np.ceil(window_ms / max(a.elapsed_time(b), 1e-3))))
    out, issue = [], []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        issue.append((time.perf_counter() - t0) * 1e3 / reps)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out)), float(np.median(issue))


def nn_encode(vp, x):
    h = F.leaky_relu(vp.bodyprior_enc_fc1(vp.bodyprior_enc_bn1(x)), 0.2)
    h = F.leaky_relu(vp.bodyprior_enc_fc2(vp.bodyprior_enc_bn2(h)), 0.2)
    return vp.bodyprior_enc_mu(h), F.softplus(vp.bodyprior_enc_logvar(h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'vposer_encode_rate.txt'))
    ap.add_argument('--sizes', default='119,100000')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'vposer_encode_rate needs the MI355X'
    dev = torch.device('cuda', 0)
    lib = _hip.get_lib()
    vp = VPoser().eval()
    vp.load_state_dict({**vp.state_dict(), **{k: torch.from_numpy(v) for k, v in {**make_vposer_weights(2), **make_vposer_enc_weights(2)}.items()}})
    vp = vp.to(dev)
    for p in vp.parameters():
        p.requires_grad_(False)
    lines = [f'vposer_encode_rate: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             'ms per call by device events: median (min .. max) of 7 runs of >= 200 ms each; [host ms to issue one call]; TFLOP/s from 655 360 FLOP per pose '
             'and pass over the event time']
    summary = []
    for B in [int(s) for s in args.sizes.split(',')]:
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, 63, generator=g) * 0.4).to(dev)
        gm, gs = torch.randn(B, 32, generator=g).to(dev), torch.randn(B, 32, generator=g).to(dev)
        w = vp._packed_enc(dev)
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        mean, std, h1, h2, lv, dx = e(B, 32), e(B, 32), e(B, 512), e(B, 512), e(B, 32), e(B, 63)
        st = lib.stream(dev)

        def c_fwd():
            lib.check(lib.vposer_encode_fwd(C.byref(w['struct']), ptr(x), 63, B, ptr(mean), ptr(std), 32, ptr(h1), ptr(h2), ptr(lv), st))

        def c_fwd_nosave():
            lib.check(lib.vposer_encode_fwd(C.byref(w['struct']), ptr(x), 63, B, ptr(mean), ptr(std), 32, None, None, None, st))

        def c_bwd():
            lib.check(lib.vposer_encode_bwd(C.byref(w['struct']), ptr(h1), ptr(h2), ptr(lv), ptr(gm), ptr(gs), 32, B, ptr(dx), 63, st))

        def m_fwd():
            with torch.no_grad():
                vp.encode(x)

        def m_fwd_bwd():
            xi = x.detach().requires_grad_(True)
            q = vp.encode(xi)
            ((q.mean * gm).sum() + (q.scale * gs).sum()).backward()

        def t_fwd():
            with torch.no_grad():
                nn_encode(vp, x)

        def t_fwd_bwd():
            xi = x.detach().requires_grad_(True)
            m, s = nn_encode(vp, xi)
            ((m * gm).sum() + (s * gs).sum()).backward()

        with torch.no_grad():                                              # the two paths compute the same thing at this size
            q, (tm, ts) = vp.encode(x), nn_encode(vp, x)
            dm = float((q.mean - tm).abs().max() / tm.abs().max())
            ds = float((q.scale - ts).abs().max() / ts.abs().max())
        lines.append(f'B = {B}: max |encode - nn modules| / max: mean {dm:.2e}, std {ds:.2e}')
        res = {}
        for name, fn, passes in (('lemo_vposer_encode_fwd alone (saves h1, h2, lv)', c_fwd, 1), ('lemo_vposer_encode_fwd alone (saves nothing)', c_fwd_nosave, 1),
                                 ('lemo_vposer_encode_bwd alone', c_bwd, 1), ('VPoser.encode, no_grad', m_fwd, 1),
                                 ('VPoser.encode + backward to Pin', m_fwd_bwd, 2), ('nn modules fp32, no_grad', t_fwd, 1),
                                 ('nn modules fp32 + autograd backward to the input', t_fwd_bwd, 2)):
            med, lo, hi, issue = timed(fn)
            res[name] = med
            tf = passes * FLOP_PER_POSE * B / (med * 1e-3) / 1e12
            lines.append(f'  {name:58s} {med:9.4f}  ({lo:.4f} .. {hi:.4f})  [{issue:.4f}]  {tf:7.2f} TFLOP/s = {100 * tf * 1e12 / PEAK:5.1f} % of the fp32 matrix peak')
        f_ratio = res['nn modules fp32, no_grad'] / res['VPoser.encode, no_grad']
        b_ratio = res['nn modules fp32 + autograd backward to the input'] / res['VPoser.encode + backward to Pin']
        summary.append(f'B = {B}: nn modules / VPoser.encode = {f_ratio:.2f} x forward, {b_ratio:.2f} x forward + backward '
                       f'({B / res["VPoser.encode, no_grad"] / 1e3:.2f} M poses/s encoded)')
    lines += summary
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
