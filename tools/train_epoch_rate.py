"""What the device-resident epoch buys per training step, on one MI355X at bs = 60: 20 steps on different batches, after 5 warm-up
steps, by device events around the whole window (host gaps included), the median of 5 windows, two paths on the same indices:
  (a) the loop the epoch replaces: per step a torch gather, the masking helper (infilling prior) and trainer.step(), which reads the
      losses back on every call;
  (b) trainer.fit_epoch(): batches assembled on the device, one captured chain replayed per step, one read-back per epoch.
Infilling prior at 210 x 135 (random-marker masking, 1 - 6 ids per step as the reference draws them), smoothness prior at
245 x 135.  Writes both times and the per-step difference to --out.
Usage: python tools/train_epoch_rate.py [--engines ae sp] [--out profiles/train_epoch_rate.txt]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lemo_amd.assets import load_assets   # noqa: E402
from lemo_amd.infill_train import InfillPriorTrainer, default_ae_state, mask_random_markers   # noqa: E402
from lemo_amd.smooth_train import SmoothPriorTrainer   # noqa: E402

BS, STEPS, WARM, WINDOWS, N = 60, 20, 5, 5, 480


def windows(fn):
    """fn(first_step, n_steps): 5 warm-up steps, then the median over 5 windows of ms per step"""
    fn(0, WARM)
    torch.cuda.synchronize()
    out = []
    for w in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(w * STEPS, STEPS)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / STEPS)
    return sorted(out)[len(out) // 2], out


def ae_paths(g):
    D, T = 208, 119
    data = torch.randn(N, 4, D, T, generator=g) * 0.5
    data[:, 0, -4:] = (torch.rand(N, 4, T, generator=g) > 0.5).float()
    data = data.cuda()
    idx = torch.stack([torch.randperm(N, generator=g)[:BS] for _ in range(WINDOWS * STEPS)])
    ids = torch.full((WINDOWS * STEPS, BS, 6), -1, dtype=torch.long)
    for s in range(len(ids)):                                     # train_infill_prior.py: n ids per STEP, drawn per image
        n = int(torch.randint(1, 7, (1,), generator=g))
        ids[s, :, :n] = (torch.rand(BS, n, generator=g) * 67).long()
    tr = InfillPriorTrainer(default_ae_state(0), batch=BS, H=D + 2, W=T + 16, lr=1e-4)
    tr.upload_dataset(data)
    idx_d, ids_d = idx.cuda(), ids.cuda()

    def loop(s0, n):
        for s in range(s0, s0 + n):
            clip = data[idx_d[s]]
            k = int((ids[s, 0] >= 0).sum())
            tr.step(mask_random_markers(clip, ids_d[s, :, :k]), clip)

    def epoch(s0, n):
        tr.fit_epoch(idx[s0:s0 + n], marker_ids=ids[s0:s0 + n])
    return tr, loop, epoch


def sp_paths(g):
    D, T = 243, 120
    data = (torch.randn(N, 1, D, T, generator=g) * 0.5).cuda()
    idx = torch.stack([torch.randperm(N, generator=g)[:BS] for _ in range(WINDOWS * STEPS)])
    tr = SmoothPriorTrainer(load_assets()['enc_w'], batch=BS, H=D + 2, W=T + 15, lr=1e-4)
    tr.upload_dataset(data)
    idx_d = idx.cuda()

    def loop(s0, n):
        for s in range(s0, s0 + n):
            tr.step(data[idx_d[s]])

    def epoch(s0, n):
        tr.fit_epoch(idx[s0:s0 + n])
    return tr, loop, epoch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--engines', nargs='+', default=['ae', 'sp'])
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'train_epoch_rate.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the MI355X'
    lines = [f'{torch.cuda.get_device_name(0)}: ms per training step at bs = {BS}, {STEPS} different batches per window after {WARM} warm-up '
             f'steps, device events around the window, median of {WINDOWS} windows (tools/train_epoch_rate.py)']
    for eng in a.engines:
        g = torch.Generator().manual_seed(7)
        tr, loop, epoch = (ae_paths if eng == 'ae' else sp_paths)(g)
        ma, wa = windows(loop)
        mb, wb = windows(epoch)
        name = 'infilling prior 210 x 135' if eng == 'ae' else 'smoothness prior 245 x 135'
        lines += [f'{name}:',
                  f'  (a) gather + mask + step() loop : {ma:8.3f} ms/step   windows {" ".join("%.3f" % v for v in wa)}',
                  f'  (b) fit_epoch                   : {mb:8.3f} ms/step   windows {" ".join("%.3f" % v for v in wb)}',
                  f'  (a) - (b)                       : {ma - mb:8.3f} ms/step ({100 * (ma - mb) / ma:.1f} % of (a))']
        tr.close()
        del tr, loop, epoch
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
