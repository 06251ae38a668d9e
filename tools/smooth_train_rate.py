"""Smoothness-prior training rate at the reference's batch: the native engine (lemo_amd.smooth_train, graph replay) next to a
torch fp32 autograd restatement of the same Enc + Dec + loss + Adam on the same GPU.  Device events; warm-up; median of several
windows.  Prints one JSON line.

    python tools/smooth_train_rate.py [--bs 60] [--windows 5] [--steps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lemo_amd.priors import DEC_IN, DEC_OUT, ENC_CHANNELS, dec_layer_keys, enc_layer_keys   # noqa: E402
from lemo_amd.smooth_train import SmoothPriorTrainer, default_dec_state, param_layout      # noqa: E402


def flop_per_step(bs, H, W):
    """2 x MACs of every 3x3 layer, forward + backward-data + weight gradient (= 3 x forward; layer 0's input gradient is
    not needed but counted as the engine skips only that one)"""
    macs = sum(ENC_CHANNELS[l] * ENC_CHANNELS[l + 1] for l in range(10)) + sum(a * b for a, b in zip(DEC_IN, DEC_OUT))
    fwd = 2 * 9 * macs * H * W
    return 3 * fwd * bs, fwd


def timed(fn, steps, windows):
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3 / steps)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=60)
    ap.add_argument('--H', type=int, default=245)
    ap.add_argument('--W', type=int, default=135)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--skip-torch', action='store_true')
    a = ap.parse_args()
    torch.manual_seed(0)
    enc = {}
    for l, k in enumerate(enc_layer_keys()):
        m = torch.nn.Conv2d(ENC_CHANNELS[l], ENC_CHANNELS[l + 1], 3, padding=1)
        enc[k + '.weight'], enc[k + '.bias'] = m.weight.detach(), m.bias.detach()
    dec = default_dec_state(1)
    x = (torch.randn(a.bs, a.H, a.W) * 0.3).cuda()
    flop, fwd = flop_per_step(a.bs, a.H, a.W)
    out = dict(bs=a.bs, H=a.H, W=a.W, flop_per_step=flop, fwd_flop_per_pixel=fwd / (a.H * a.W))

    tr = SmoothPriorTrainer(enc, dec, batch=a.bs, H=a.H, W=a.W, device='cuda')
    step = lambda: tr.lib.check(tr.lib.sptrain_step(tr.h, x.data_ptr(), 1, None, tr._s()), 'sptrain_step')
    torch.cuda.synchronize()
    with torch.cuda.stream(tr.stream):                   # the engine's own stream: events recorded where it runs
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t, ts = timed(step, a.steps, a.windows)
    out.update(engine_s_per_step=t, engine_steps_per_s=1 / t, engine_tflops=flop / t / 1e12, engine_windows=ts)
    tr.close()
    del tr
    torch.cuda.empty_cache()

    if not a.skip_torch:
        ps = {k: v.cuda().clone().requires_grad_(True) for k, v in list(enc.items()) + list(dec.items())}
        opt = torch.optim.Adam([ps[k] for k, _ in param_layout()], lr=1e-4)

        def tstep():
            opt.zero_grad()
            h = x.unsqueeze(1)
            for k in enc_layer_keys():
                h = F.leaky_relu(F.conv2d(h, ps[k + '.weight'], ps[k + '.bias'], padding=1), 0.2)
            z = h
            for j, k in enumerate(dec_layer_keys()):
                h = F.conv_transpose2d(h, ps[k + '.weight'], ps[k + '.bias'], stride=1, padding=1)
                if j != 9:
                    h = F.leaky_relu(h, 0.2)
            loss = F.l1_loss(x.unsqueeze(1), h) + 1000.0 * torch.mean((z[..., 1:] - z[..., :-1]) ** 2)
            loss.backward()
            opt.step()
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False
        for _ in range(3):
            tstep()
        torch.cuda.synchronize()
        t2, ts2 = timed(tstep, a.steps, a.windows)
        out.update(torch_fp32_s_per_step=t2, torch_fp32_steps_per_s=1 / t2, torch_fp32_tflops=flop / t2 / 1e12, torch_windows=ts2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
