"""Emit the fixture of the VPoser encoder tests: the reference's own ``VPoser`` class (human_body_prior/train/vposer_smpl.py, imported
from where it lies through ref_harness; nothing is copied) in eval(), with the seeded weights make_vposer_weights(2) +
make_vposer_enc_weights(2), on B = 33 axis-angle poses of sigma 0.4.

Run ONLY in the build container (needs the reference tree; it never travels to the GPU box):

    python tests/golden/make_vposer_encode.py

vposer_encode.npz (arrays only):
  Pin [33, 1, 21, 3]; mean, std [33, 32] = encode(Pin).mean / .scale; pose_aa [33, 1, 21, 3] = forward(Pin, output_type='aa')['pose_aa'] under
  torch.manual_seed(SEED); z [33, 32] = the latent sample that forward drew, obtained by re-seeding and calling encode(Pin).rsample();
  eps [33, 32] float64 = (z - mean) / std in float64, so that mean + std * eps reproduces the draw.
vposer_encode_vs_reference.txt: the distance (max |a - b| / max |b|) of the float32 and of the float64 restatement
(tests/vposer_enc_common.py::restate, then oracle.lemo_oracle.vposer_decode) from the reference's arrays.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import ref_harness as RH                                              # noqa: E402
import vposer_enc_common as K                                         # noqa: E402
from lemo_amd.vposer import make_vposer_enc_weights, make_vposer_weights   # noqa: E402
from oracle import lemo_oracle as O                                   # noqa: E402

B, SEED = 33, 1234


def main():
    dw, ew = make_vposer_weights(2), make_vposer_enc_weights(2)
    vp = RH.ref_vposer({k: torch.from_numpy(v) for k, v in {**dw, **ew}.items()})
    assert not vp.training
    Pin = K.poses(B, 2024).view(B, 1, 21, 3)
    with torch.no_grad():
        q = vp.encode(Pin)
        torch.manual_seed(SEED)
        res = vp(Pin, output_type='aa')
        torch.manual_seed(SEED)
        z = vp.encode(Pin).rsample()
    assert torch.equal(res['mean'], q.mean) and torch.equal(res['std'], q.scale)
    eps = (z.double() - q.mean.double()) / q.scale.double()
    np.savez_compressed(os.path.join(HERE, 'vposer_encode.npz'), Pin=Pin.numpy(), mean=q.mean.numpy(), std=q.scale.numpy(),
                        pose_aa=res['pose_aa'].numpy(), z=z.numpy(), eps=eps.numpy())
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    lines = []
    for name, dtype in (('float32', torch.float32), ('float64', torch.float64)):
        with torch.no_grad():
            r = K.restate(ew, Pin.view(B, 63), dtype)
            aa = O.vposer_decode({k: torch.from_numpy(v).to(dtype) for k, v in dw.items()}, r['mean'] + r['std'] * eps.to(dtype), 'aa')
        lines += [f'VPoser.encode.mean    {name} restatement vs reference  {rel(r["mean"], q.mean):.3e}',
                  f'VPoser.encode.std     {name} restatement vs reference  {rel(r["std"], q.scale):.3e}',
                  f'VPoser.forward.pose_aa {name} restatement vs reference  {rel(aa, res["pose_aa"]):.3e}']
    with open(os.path.join(HERE, 'vposer_encode_vs_reference.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    torch.set_num_threads(16)
    main()
