"""One training step of the infilling prior in torch (lemo_amd.infill_torch), as the lemo_aetrain_* tests use it: gradients, Adam
steps and the gates they are held to."""
import torch

from lemo_amd.infill_torch import ae_forward, losses  # noqa: F401
from lemo_amd.infill_train import param_layout


def step(sd, x, y, weights=(10., 10., 1.), dtype=torch.float64, winners=None):
    """one forward / backward -> (losses (L_body, L_v, L_c, total) as floats, {key: gradient}); winners: ae_forward's"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    rec = ae_forward(p, x.to(dtype), winners)
    lb, lv, lc = losses(rec, y.to(dtype))
    tot = weights[0] * lb + weights[1] * lv + weights[2] * lc
    tot.backward()
    return [float(lb.detach()), float(lv.detach()), float(lc.detach()), float(tot.detach())], {k: p[k].grad.detach() for k, _ in param_layout()}


def train(sd, x, y, steps, lr, weights=(10., 10., 1.), dtype=torch.float64):
    """`steps` reference steps (torch.optim.Adam) -> (per-step losses, the final state)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam([p[k] for k, _ in param_layout()], lr=lr)
    hist = []
    for _ in range(steps):
        opt.zero_grad()
        rec = ae_forward(p, x.to(dtype))
        lb, lv, lc = losses(rec, y.to(dtype))
        tot = weights[0] * lb + weights[1] * lv + weights[2] * lc
        tot.backward()
        opt.step()
        hist.append([float(lb.detach()), float(lv.detach()), float(lc.detach()), float(tot.detach())])
    return hist, {k: v.detach() for k, v in p.items()}


def flat(d):
    return torch.cat([d[k].reshape(-1).double().cpu() for k, _ in param_layout()])


def per_tensor_gate(got, want, rel=2e-5, ref32=None):
    """max |got - want| per tensor vs rel * max |want|, or 2 x the distance of a torch fp32 computation `ref32` where that is
    larger (gradients that are sums of many cancelling terms) -> list of failures"""
    bad = []
    for k, _ in param_layout():
        g, w = got[k].double().cpu(), want[k].double().cpu()
        err, tol = float((g - w).abs().max()), rel * float(w.abs().max()) + 1e-30
        if ref32 is not None:
            tol = max(tol, 2 * float((ref32[k].double().cpu() - w).abs().max()))
        if err > tol:
            bad.append((k, err, tol))
    return bad


def sign_flip_gate(got, want, lr, steps):
    """parameters after `steps` Adam steps: an entry may differ by at most 2 lr steps (its update's sign flipped where the gradient
    is near zero), and only a small fraction may differ by more than 1 % of lr"""
    d = (flat(got) - flat(want)).abs()
    return float(d.max()) <= 2 * lr * steps and float((d > 0.01 * lr).double().mean()) <= 1e-3
