"""Emit the fixture of the infilling-prior training tests: the reference's own training step (train_infill_prior.py:185-203 with
models/AE.py AE(downsample=True, in_channel=4, kernel=3), imported from where it lies; nothing is copied), in float64.

Run ONLY in the build container (needs the reference tree; it never travels to the GPU box):

    python tests/golden/make_infill_train.py

infill_train.npz: the per-tensor sums of default_ae_state(1234) (the init the reference class is loaded with); a seeded bs = 2 batch
of clip images [2, 4, 208, 119] as fp16 (values exact in fp16), image 0 masked by mask_random_markers, image 1 by mask_prox with the
first PROX mask clip of the reference's mask_markers/; the 4 losses (L_body, L_v, L_c, total) of each of 3 Adam steps (lr 1e-4);
per tensor the step-1 max |gradient|, and at up to SAMPLE seeded entries per tensor the step-1 gradient and the parameter change
after 3 steps.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = '/root/reference'
sys.path.insert(0, ROOT)

from lemo_amd.infill_train import (default_ae_state, flatten_state, load_prox_mask_clips, mask_prox,   # noqa: E402
                                   mask_random_markers, param_layout)

SAMPLE = 1024
D, T = 208, 119


def clips(bs=2, seed=2025):
    g = np.random.default_rng(seed)
    acc = g.standard_normal((bs, 4, D, T + 40))
    k = np.exp(-0.5 * (np.arange(-12, 13) / 5.0) ** 2)
    acc = np.apply_along_axis(lambda r: np.convolve(r, k / k.sum(), 'same'), -1, acc)
    pos = np.cumsum(np.cumsum(acc, -1), -1)[..., 20:20 + T] * 1e-3 + g.standard_normal((bs, 4, D, 1))
    pos = (pos - pos.mean((0, 3), keepdims=True)) / (pos.std((0, 3), keepdims=True) + 1e-8)
    pos[:, 0, -4:] = (g.random((bs, 4, T)) > 0.5)                    # foot-contact labels
    return torch.from_numpy(pos.astype(np.float16).astype(np.float32))


def main():
    sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
    sys.path.insert(0, REF)
    from models.AE import AE                                        # reference class
    sd0 = default_ae_state(1234)
    model = AE(downsample=True, in_channel=4, kernel=3).double()
    model.load_state_dict({k: v.double() for k, v in sd0.items()})
    w0 = flatten_state(sd0)
    clip_img = clips()
    ids = torch.tensor([[16, 5, 40]])
    prox = load_prox_mask_clips(os.path.join(REF, 'mask_markers'))
    inp = torch.cat([mask_random_markers(clip_img[:1], ids), mask_prox(clip_img[1:], prox[:1])])
    assert torch.equal(inp.half().float(), inp)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    bce = nn.BCEWithLogitsLoss()
    losses, grad1 = [], None
    for step in range(3):                                          # train_infill_prior.py:185-203
        opt.zero_grad()
        x = F.pad(inp.double(), (8, 8, 1, 1), 'reflect')
        ci = F.pad(clip_img.double(), (8, 8, 1, 1), 'reflect')
        rec, z = model(x)
        civ = ci[:, :, :, 1:] - ci[:, :, :, 0:-1]
        recv = rec[:, :, :, 1:] - rec[:, :, :, 0:-1]
        lb = F.l1_loss(ci[:, 0, 0:-5], rec[:, 0, 0:-5])
        lv = F.l1_loss(civ[:, 0, 0:-5], recv[:, 0, 0:-5])
        lc = bce(rec[:, 0, -5:], ci[:, 0, -5:])
        loss = 10. * lb + 10. * lv + 1. * lc
        loss.backward()
        if step == 0:
            named = dict(model.named_parameters())
            grad1 = np.concatenate([named[k].grad.numpy().ravel() for k, _ in param_layout()])
        opt.step()
        losses.append([float(lb.detach()), float(lv.detach()), float(lc.detach()), float(loss.detach())])
    w3 = flatten_state({k: v.detach() for k, v in model.state_dict().items()})
    rng = np.random.default_rng(7)
    idx, o, gmax = [], 0, []
    for k, shp in param_layout():
        n = int(np.prod(shp))
        sel = np.arange(n) if n <= SAMPLE else np.sort(rng.choice(n, SAMPLE, replace=False))
        idx.append(o + sel)
        gmax.append(np.abs(grad1[o:o + n]).max())
        o += n
    idx = np.concatenate(idx)
    np.savez_compressed(os.path.join(HERE, 'infill_train.npz'), clip_img=clip_img.numpy().astype(np.float16),
                        clip_img_input=inp.numpy().astype(np.float16),
                        init_sums=np.array([float(sd0[k].double().sum()) for k, _ in param_layout()]),
                        losses=np.array(losses), idx=idx.astype(np.int32), grad1=grad1[idx].astype(np.float64),
                        gmax=np.array(gmax, np.float64), dw3=(w3.astype(np.float64) - w0.astype(np.float64))[idx], lr=np.float64(1e-4))
    print('losses', losses)


if __name__ == '__main__':
    torch.set_num_threads(16)
    main()
