"""Float64 restatement of the smoothness-prior training step (models/AE_sep.py Enc + Dec with downsample=False,
train_smooth_prior.py:96-136) shared by the emulator and GPU tests of lemo_amd.smooth_train."""
import numpy as np
import torch
import torch.nn.functional as F

from lemo_amd.priors import dec_layer_keys, enc_layer_keys
from lemo_amd.smooth_train import param_layout


def random_state(seed, scale=1.0):
    """Enc + Dec state dicts with torch-default-like magnitudes (uniform, bound 1/sqrt(fan_in))"""
    g = torch.Generator().manual_seed(seed)
    enc, dec = {}, {}
    for k, shp in param_layout():
        bound = scale / np.sqrt(shp[1] * 9) if len(shp) == 4 else 0.1 * scale     # fan_in = weight.size(1) * 9 (Conv2d and ConvTranspose2d)
        t = (torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * bound
        (enc if k.startswith('enc_') else dec)[k] = t.float()
    return enc, dec


def forward_loss(enc, dec, x, w_rec=1.0, w_smooth=1000.0):
    """x [bs, H, W] -> (loss, loss_rec, loss_smooth, rec, z) in x's dtype; enc / dec: tensors of that dtype"""
    h = x.unsqueeze(1)
    for k in enc_layer_keys():
        h = F.leaky_relu(F.conv2d(h, enc[k + '.weight'], enc[k + '.bias'], padding=1), 0.2)
    z = h
    for j, k in enumerate(dec_layer_keys()):
        h = F.conv_transpose2d(h, dec[k + '.weight'], dec[k + '.bias'], stride=1, padding=1)
        if j != 9:
            h = F.leaky_relu(h, 0.2)
    rec = h
    l_rec = F.l1_loss(x.unsqueeze(1), rec)
    l_sm = torch.mean((z[..., 1:] - z[..., :-1]) ** 2)
    return w_rec * l_rec + w_smooth * l_sm, l_rec, l_sm, rec, z


def grads(enc, dec, x, dtype=torch.float64, **kw):
    """(losses (rec, smooth), {key: gradient}) of one step, evaluated in `dtype`"""
    e = {k: v.to(dtype).clone().requires_grad_(True) for k, v in enc.items()}
    d = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dec.items()}
    loss, lr_, ls, _, _ = forward_loss(e, d, x.to(dtype), **kw)
    loss.backward()
    g = {k: v.grad.detach() for k, v in list(e.items()) + list(d.items())}
    return (float(lr_.detach()), float(ls.detach())), g


def train(enc, dec, x, steps, lr=1e-4, dtype=torch.float64, **kw):
    """`steps` Adam steps (torch.optim.Adam, default betas / eps) -> (list of (loss_rec, loss_smooth), final {key: param})"""
    ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in list(enc.items()) + list(dec.items())}
    opt = torch.optim.Adam([ps[k] for k, _ in param_layout()], lr=lr)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        loss, lr_, ls, _, _ = forward_loss({k: ps[k] for k in enc}, {k: ps[k] for k in dec}, x.to(dtype), **kw)
        loss.backward()
        opt.step()
        out.append((float(lr_.detach()), float(ls.detach())))
    return out, {k: v.detach() for k, v in ps.items()}


def flat(d):
    return torch.cat([d[k].reshape(-1).to(torch.float64) for k, _ in param_layout()])


def per_tensor_gate(got, want, rel=2e-5, floor=None):
    """max |got - want| per tensor vs rel * max |want| (or the given per-tensor floor where that is larger); -> list of failures"""
    bad = []
    for k, _ in param_layout():
        g, w = got[k].to(torch.float64), want[k].to(torch.float64)
        err = float((g - w).abs().max())
        tol = rel * float(w.abs().max()) + 1e-30
        if floor is not None:
            tol = max(tol, floor[k])
        if err > tol:
            bad.append((k, err, tol))
    return bad
