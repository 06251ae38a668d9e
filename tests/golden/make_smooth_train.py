"""Emit the fixtures of the smoothness-prior training tests: the reference's own training step (train_smooth_prior.py:96-136 with
models/AE_sep.py Enc + Dec, imported from where they lie; nothing is copied) on the runs/15217 weights.

Run ONLY in the build container (needs the reference tree; it never travels to the GPU box):

    python tests/golden/make_smooth_train.py

smooth_dec_15217.npz: runs/15217/Dec_last_model.pkl as {state_dict key: float32 array} (the Enc half is the shipped asset
lemo_amd/assets/smooth_enc_15217.npz; asserted equal to Enc_last_model.pkl here).
smooth_train.npz: a seeded bs = 2 batch of clip images [2, 1, 243, 120] (smooth random marker trajectories, per-row normalised),
the losses of 3 Adam steps (lr 1e-4), Dec(Enc(x)) of clip 0, and -- to keep the file small -- for every one of the 40 tensors its
max |gradient| of step 1 plus the step-1 gradient and the parameter change after 3 steps (dw3 = w3 - w0) at up to SAMPLE
seeded entries (all entries of the smaller tensors); everything evaluated in float64 by the reference classes.  Full-tensor
gradient parity is the float64-restatement test's job (tests/test_smooth_train_gpu.py).
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = '/root/reference'
sys.path.insert(0, ROOT)

from lemo_amd.assets import load_smooth_encoder_weights              # noqa: E402
from lemo_amd.smooth_train import flatten_state, param_layout      # noqa: E402

SAMPLE = 1024


def clips(bs=2, d=243, T=120, seed=2024):
    g = np.random.default_rng(seed)
    acc = g.standard_normal((bs, d, T + 40))
    k = np.exp(-0.5 * (np.arange(-12, 13) / 5.0) ** 2)
    acc = np.stack([[np.convolve(r, k / k.sum(), 'same') for r in c] for c in acc])
    pos = np.cumsum(np.cumsum(acc, -1), -1)[..., 20:20 + T] * 1e-3 + g.standard_normal((bs, d, 1))
    pos = (pos - pos.mean((0, 2), keepdims=True)) / (pos.std((0, 2), keepdims=True) + 1e-8)
    return torch.from_numpy(pos[:, None].astype(np.float32))


def main():
    sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
    sys.path.insert(0, REF)
    from models.AE_sep import Dec, Enc                                # reference classes
    enc = Enc(downsample=False, z_channel=64).double()
    dec = Dec(downsample=False, z_channel=64).double()
    esd = torch.load(f'{REF}/runs/15217/Enc_last_model.pkl', map_location='cpu')
    dsd = torch.load(f'{REF}/runs/15217/Dec_last_model.pkl', map_location='cpu')
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    shipped = load_smooth_encoder_weights()
    assert all(np.array_equal(shipped[k], v.numpy()) for k, v in esd.items())
    w0 = flatten_state(esd, dsd)
    clip_img = clips()
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=1e-4)
    losses, grad1 = [], None
    for step in range(3):                                             # train_smooth_prior.py:109-136
        opt.zero_grad()
        x = clip_img.double()
        v = F.pad(x[..., 1:] - x[..., :-1], (8, 8, 1, 1), 'reflect')
        z, *sizes = enc(v)
        rec = dec(z, *sizes)
        l_rec = F.l1_loss(v, rec)
        l_sm = torch.mean((z[..., 1:] - z[..., :-1]) ** 2)
        (1.0 * l_rec + 1000.0 * l_sm).backward()
        if step == 0:
            sd = {n: p.grad for n, p in list(('enc.' + a, b) for a, b in enc.named_parameters()) + list(('dec.' + a, b) for a, b in dec.named_parameters())}
            grad1 = np.concatenate([sd[('enc.' if k.startswith('enc_') else 'dec.') + k].numpy().ravel() for k, _ in param_layout()])
            with torch.no_grad():
                dec_enc = rec[0, 0].numpy()
        opt.step()
        losses.append([float(l_rec.detach()), float(l_sm.detach())])
    w3 = flatten_state({k: v.detach() for k, v in enc.state_dict().items()}, {k: v.detach() for k, v in dec.state_dict().items()})
    rng = np.random.default_rng(7)
    idx, o, gmax = [], 0, []
    for k, shp in param_layout():
        n = int(np.prod(shp))
        sel = np.arange(n) if n <= SAMPLE else np.sort(rng.choice(n, SAMPLE, replace=False))
        idx.append(o + sel)
        gmax.append(np.abs(grad1[o:o + n]).max())
        o += n
    idx = np.concatenate(idx)
    np.savez_compressed(os.path.join(HERE, 'smooth_dec_15217.npz'), **{k: v.numpy().astype(np.float32) for k, v in dsd.items()})
    np.savez_compressed(os.path.join(HERE, 'smooth_train.npz'), clip_img=clip_img.numpy(), losses=np.array(losses),
                        idx=idx.astype(np.int32), grad1=grad1[idx].astype(np.float64), gmax=np.array(gmax, np.float64),
                        dw3=(w3.astype(np.float64) - w0.astype(np.float64))[idx], dec_enc0=dec_enc.astype(np.float32),
                        lr=np.float64(1e-4))
    print('losses', losses)


if __name__ == '__main__':
    torch.set_num_threads(16)
    main()
