"""The encoder's turn launch (lemo_conv3x3_turn_f16: layer 9 forward, the smoothness-loss gradient, layer 9 backward-data) against
float64, shared by tests/test_turn_emu.py (host-emulated build) and tests/test_turn_gpu.py (MI355X).

One case checks:
  1. z = act[10] elementwise against float64 (tests/conv_shapes_common.py's split-f16 tau times |x| (*) |w| + |b|, plus its
     max-relative gate);
  2. d(pre-act 10) (the kernel's debug copy) bit-identical to lemo_smooth_loss applied to the kernel's own z.  The input has two
     channels, one per staging phase, held at 1.0 and every other |x| < 1, so every workgroup stages with the same power-of-two scales
     and the halo z values it recomputes equal its neighbours' published ones bit for bit;
  3. d(pre-act 9) elementwise against float64, the bound chaining the z error through the stencil and layer 9's adjoint;
  4. the smoothness sum of squares against float64, and only element 0 of each accumulator slot written;
  5. NaN sentinels on the borders of z, d(pre-act 9), d(pre-act 10) and past their ends stay untouched;
  6. two launches give identical bits;
  7. refused shapes return LEMO_ERR_SHAPE and write nothing."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_shapes_common as C
from lemo_amd._hip import ptr
from lemo_amd.assets import load_assets
from lemo_amd.priors import enc_layer_keys, pack_conv3x3_split_f16, pack_conv3x3_bwd_split_f16, to_cg8p, from_cg8p

SMOOTH_W = 0.5                   # any loss weight: coef2 = weight * 2 / (C H (W - 1)), as the fit engine forms it


def layer9():
    """the encoder's last 64 -> 64 layer (runs/15217)"""
    A = load_assets()['enc_w']
    k = [k for k in enc_layer_keys() if np.asarray(A[k + '.weight']).shape[:2] == (64, 64)][-1]
    return (torch.from_numpy(np.asarray(A[k + '.weight'], np.float32).copy()),
            torch.from_numpy(np.asarray(A[k + '.bias'], np.float32).copy()))


def turn_input(H, W, seed):
    """act[9]-like input [64, H, W]: |x| < 1 except channels 0 and 16 (one per staging phase), held at 1.0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(64, H, W, generator=g)
    x = (torch.where(x > 0, x, 0.2 * x) * 0.3).clamp(-0.99, 0.99)
    x[0] = 1.0
    x[16] = 1.0
    return x


def stencil64(z, W, coef2):
    """float64 d(pre-act 10) from z [64, H, W] and the magnitude of its error propagated from |z| errors: (dpre, |stencil| weights)"""
    c, l, r = z, F.pad(z, (1, 0))[..., :-1], F.pad(z, (0, 1))[..., 1:]
    hasl = torch.arange(W) >= 1
    hasr = torch.arange(W) <= W - 2
    gr = torch.where(hasl, c - l, 0.0) - torch.where(hasr, r - c, 0.0)
    g = torch.where(z > 0, 1.0, 0.2).double()
    return coef2 * gr * g, g, hasl, hasr


def run_turn(lib, dev, H, W, seed=0):
    what = f'turn at {H} x {W}'
    w, b = layer9()
    (pf, iF), (pb, iB) = pack_conv3x3_split_f16(w.numpy()), pack_conv3x3_bwd_split_f16(w.numpy())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    wf, wb = t(pf.view(np.int16)), t(pb.view(np.int16))
    coef2 = float(np.float32(SMOOTH_W * 2.0 / (64 * max(H, 1) * max(W - 1, 1))))
    s = lib.stream(dev)
    x = turn_input(H, W, seed=H * 131 + W + seed)
    xin, bias = to_cg8p(x).to(dev), b.to(dev)
    outs = []
    for _ in range(2):
        wz, z = C.sentinel_cg8p(64, H, W, dev)
        wo, o = C.sentinel_cg8p(64, H, W, dev)
        wd, d = C.sentinel_cg8p(64, H, W, dev)
        acc = torch.zeros(32 * 16 + 64, dtype=torch.float64, device=dev)
        outs.append((wz, z, wo, o, wd, d, acc))
    if lib.conv3x3_turn_supported(H, W) != 1:
        wz, z, wo, o, wd, d, acc = outs[0]
        rc = lib.conv3x3_turn_f16(ptr(xin), ptr(wf), iF, ptr(bias), ptr(wb), iB, ptr(z), ptr(o), ptr(acc), coef2, H, W, ptr(d), None, s)
        C._sync(lib)
        assert rc == C.ERR_SHAPE, f'{what}: expected a refusal, got {rc}'
        for buf in (wz, wo, wd):
            assert torch.isnan(buf.cpu()).all(), f'{what}: a refused launch wrote'
        assert (acc.cpu() == 0).all(), f'{what}: a refused launch accumulated'
        return None
    for wz, z, wo, o, wd, d, acc in outs:
        lib.check(lib.conv3x3_turn_f16(ptr(xin), ptr(wf), iF, ptr(bias), ptr(wb), iB, ptr(z), ptr(o), ptr(acc), coef2, H, W, ptr(d), None, s),
                  what)
    C._sync(lib)
    wz, z, wo, o, wd, d, acc = outs[0]
    for (a1, a2, name) in ((wz, outs[1][0], 'z'), (wo, outs[1][2], 'd(pre-act 9)'), (wd, outs[1][4], 'd(pre-act 10)')):
        C.check_cg8p_write_set(a1, 64, H, W, f'{what} ({name})')
        C.same_bits(a1, a2, f'{what} ({name})')
    C.same_bits(acc.float(), outs[1][6].float(), what + ' (loss accumulator)')

    # 1. z against float64
    zref, zmag = C.ref_layer(x, w, b, 0)
    zgot = from_cg8p(z.cpu(), H, W)
    r_z = C.check_close(zgot, zref, zmag, 'split_f16', what + ' (z)')

    # 2. d(pre-act 10) bit-identical to lemo_smooth_loss on the kernel's own z
    wsd, sd = C.sentinel_cg8p(64, H, W, dev)
    part = torch.zeros(lib.smooth_loss_blocks(H, W, 64) + 16, dtype=torch.float32, device=dev)
    lib.check(lib.smooth_loss(ptr(z), ptr(sd), ptr(part), H, W, 64, coef2, s), what + ' (lemo_smooth_loss)')
    C._sync(lib)
    dgot, dsm = from_cg8p(d.cpu(), H, W), from_cg8p(sd.cpu(), H, W)
    if not torch.equal(dgot.view(torch.int32), dsm.view(torch.int32)):
        bad = (dgot.view(torch.int32) != dsm.view(torch.int32)).nonzero()
        raise AssertionError(f'{what}: d(pre-act 10) differs from lemo_smooth_loss on the published z at {bad.shape[0]} entries, '
                             f'first {tuple(bad[0].tolist())}')

    # 3. d(pre-act 9) against float64: the z error (tau * zmag per value) enters the stencil with |coefficients| 2, 1, 1
    d10, g10, hasl, hasr = stencil64(zref, W, coef2)
    zm_l, zm_r = F.pad(zmag, (1, 0))[..., :-1], F.pad(zmag, (0, 1))[..., 1:]
    m10 = abs(coef2) * g10 * (torch.where(hasl, zmag + zm_l, 0.0) + torch.where(hasr, zmag + zm_r, 0.0))
    g9 = C.lrelu_d(x)
    ref9 = F.conv_transpose2d(d10[None], w.double(), padding=1)[0] * g9
    mag9 = F.conv_transpose2d((m10 + d10.abs())[None], w.double().abs(), padding=1)[0] * g9
    r_9 = C.check_close(from_cg8p(o.cpu(), H, W), ref9, mag9, 'split_f16', what + ' (d(pre-act 9))')

    # 4. the loss partials: sum over slots vs float64; only element 0 of each slot, nothing past the 32 slots
    a = acc.cpu()
    slots = a[:512].view(32, 16)
    assert (slots[:, 1:] == 0).all() and (a[512:] == 0).all(), f'{what}: wrote outside the slots\' element 0'
    sq64 = float(((zref[..., 1:] - zref[..., :-1]) ** 2).sum())
    got = float(slots[:, 0].sum())
    assert abs(got - sq64) <= 1e-5 * sq64 + 1e-30, f'{what}: sum of squares {got!r} vs float64 {sq64!r}'
    return r_z, r_9


# ---------------------------------------------------------------------------------------------------------------------------
# the fit engine: lemo_fit_step (the turn schedule, conv variant 9) against lemo_fit_forward (layer 9 + fit_losses) + lemo_fit_backward
# (the turn launch without losses, then the same chain as the step)

LOSS_REL = 1e-6                  # the per-frame and smoothness sums are taken in another order by the turn launch


def make_fitter(prob, markers, dev, lib, turn, monkeypatch):
    """an AmassTemporalFitter on the problem; `turn` sets LEMO_ENC_TURN, which the engine reads when it is created"""
    from lemo_amd.fitting import AmassTemporalFitter
    monkeypatch.setenv('LEMO_ENC_TURN', '1' if turn else '0')
    f = AmassTemporalFitter(prob['model'], prob['vposer_w'], prob['enc_w'], prob['ids'], prob['Xmean'], prob['Xstd'], prob['B'], dev,
                            lib=lib)
    f.load_sequence(prob['seq']['init_params'], markers, prob['seq']['contact_lbl'])
    monkeypatch.delenv('LEMO_ENC_TURN')
    return f


def step_vs_forward_backward(prob, markers, dev, lib, monkeypatch, use_graph=False):
    """one `step` against `forward` + `backward` from the same state: every loss within LOSS_REL (the forward's come from layer 9 +
    fit_losses, the step's from the turn launch), the gradients bit for bit (both run the turn launch and the same backward chain: the
    Adam check of tests/test_gpu_teacher.py takes forward + backward's gradient for the step's).  Returns the worst loss ratio."""
    ref = make_fitter(prob, markers, dev, lib, True, monkeypatch)
    ref.forward()
    ref.backward()
    L0, g0 = ref.losses(), {k: v.detach().clone() for k, v in ref.grads().items()}
    f = make_fitter(prob, markers, dev, lib, True, monkeypatch)
    f.step(1, use_graph=use_graph)
    L1, g1 = f.losses(), f.grads()
    wl = 0.0
    for k in L0:
        r = abs(L1[k] - L0[k]) / max(abs(L0[k]), 1e-30)
        assert r <= LOSS_REL, f'loss {k}: step {L1[k]!r} vs forward + backward {L0[k]!r}'
        wl = max(wl, r)
    for k in g0:
        a, b = g1[k].cpu(), g0[k].cpu()
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, b), f'gradient {k}: step vs forward + backward, max diff {float((a - b).abs().max()):.3e}'
    return wl
