"""Rate of the infilling-prior training step (lemo_aetrain_*, InfillPriorTrainer) at 210 x 135: device-event time per step, the median
of 5 windows of 5 steps, at bs = 60 and 120, next to torch fp32 autograd + torch.optim.Adam on the same GPU (TF32 off).  One JSON
line per measurement.  Usage: python tools/infill_train_rate.py [--bs 60 120] [--torch 1]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lemo_amd import infill_torch as R   # noqa: E402
from lemo_amd.infill_train import InfillPriorTrainer, default_ae_state, network_tensors   # noqa: E402

H, W, D, T = 210, 135, 208, 119


def flops_per_step(bs):
    """3 x the forward's multiply-adds x 2 (forward, backward-data, weight gradient), from the layer shapes"""
    h, w = [H], [W]
    for _ in range(5):
        h.append((h[-1] - 1) // 2 + 1)
        w.append((w[-1] - 1) // 2 + 1)
    enc = [(4, 32), (32, 64), (64, 128), (128, 256), (256, 256)]
    dec = [(256, 256), (256, 128), (128, 64), (64, 32), (32, 1)]
    macs = 0
    for b, (ci, co) in enumerate(enc):
        macs += h[b] * w[b] * 9 * (ci * co + co * co)
    for b, (ci, co) in enumerate(dec):
        macs += h[4 - b] * w[4 - b] * 9 * (ci * co + co * co)
    return 3 * 2 * macs * bs


def timed(fn, windows=5, per=5):
    fn(1)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(per)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / per)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[60, 120])
    ap.add_argument('--torch', type=int, default=1)
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    for bs in a.bs:
        g = torch.Generator().manual_seed(bs)
        img = (torch.randn(bs, 4, D, T, generator=g) * 0.5).cuda()
        inp = img.clone()
        inp[:, 0, 3:12] = 0.
        sd = default_ae_state(0)
        tr = InfillPriorTrainer(sd, batch=bs, H=H, W=W, lr=1e-4)
        x, y = network_tensors(inp, img)
        ms = timed(lambda n: tr.step(x, y, n=n, prepared=True))
        fl = flops_per_step(bs)
        rec = {'what': 'engine', 'bs': bs, 'H': H, 'W': W, 'ms_per_step': round(ms, 3), 'tflops': round(fl / ms / 1e9, 2),
               'tflop_per_step': round(fl / 1e12, 3), 'ws_gib': round(tr.ws.numel() * 4 / 2 ** 30, 3)}
        print(json.dumps(rec), flush=True)
        tr.close()
        if a.torch:
            p = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
            opt = torch.optim.Adam(list(p.values()), lr=1e-4)

            def tstep(n):
                for _ in range(n):
                    opt.zero_grad()
                    lb, lv, lc = R.losses(R.ae_forward(p, x), y)
                    (10 * lb + 10 * lv + lc).backward()
                    opt.step()
            tms = timed(tstep)
            print(json.dumps({'what': 'torch_fp32_autograd', 'bs': bs, 'ms_per_step': round(tms, 3), 'tflops': round(fl / tms / 1e9, 2),
                              'engine_speedup': round(tms / ms, 3)}), flush=True)
            del p, opt
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
