"""GPU suite: the smoothness-prior training engine (lemo_sptrain_*) against the reference's own training step
(tests/golden/smooth_train.npz + smooth_dec_15217.npz, made by tests/golden/make_smooth_train.py; the Enc weights are the shipped
asset), a float64 restatement, torch fp32 on the same GPU, and itself (graph replay vs eager, engine vs engine)."""
import os

import numpy as np
import pytest
import torch

import sptrain_common as R
from lemo_amd import priors
from lemo_amd.assets import load_smooth_encoder_weights
from lemo_amd.smooth_train import SmoothPriorTrainer, flatten_state, network_input, param_layout, unflatten_state

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = [k for k, _ in param_layout()]


def _fix():
    f = np.load(os.path.join(GOLDEN, 'smooth_train.npz'))
    d = np.load(os.path.join(GOLDEN, 'smooth_dec_15217.npz'))
    enc = {k: torch.from_numpy(v) for k, v in load_smooth_encoder_weights().items()}
    dec = {k: torch.from_numpy(d[k]) for k in d.files}
    return f, enc, dec


def _fp32_floor(enc, dec, x, want):
    """2 x the distance of torch fp32 on the CPU from the float64 gradient, per tensor"""
    _, g32 = R.grads(enc, dec, x, dtype=torch.float32)
    return {k: 2.0 * float((g32[k].double() - want[k].double()).abs().max()) for k in KEYS}


def _sampled_gate(got_flat, want, idx, gmax, floor_flat, rel=2e-5):
    """the per-tensor gradient gate on the fixture's sampled entries: |got - want| <= max(rel * max |want| over the WHOLE tensor,
    2 x torch fp32's distance on the same entries); -> list of failures"""
    bad, o = [], 0
    for t, (k, shp) in enumerate(param_layout()):
        n = int(np.prod(shp))
        m = (idx >= o) & (idx < o + n)
        err = float(np.abs(got_flat[idx[m]] - want[m]).max())
        tol = max(rel * gmax[t], 2.0 * float(np.abs(floor_flat[idx[m]] - want[m]).max()))
        if err > tol:
            bad.append((k, err, tol))
        o += n
    return bad


@pytest.mark.timeout(300)
def test_fixture_parity_losses_gradients_and_three_adam_steps():
    f, enc, dec = _fix()
    clip = torch.from_numpy(f['clip_img'])
    dev = torch.device('cuda')
    tr = SmoothPriorTrainer(enc, dec, batch=2, H=245, W=135, lr=1e-4, device=dev)
    want_l = f['losses']
    x = network_input(clip)
    # loss floor: torch fp32 (CPU) of the same step, x 2
    l32, g32 = R.grads(enc, dec, x, dtype=torch.float32)
    got = []
    for step in range(3):
        got.append(tr.step(clip.to(dev)))
        if step == 0:
            g1 = unflatten_state(tr.flat_grads().numpy())
    for i in range(2):
        tol = max(1e-5 * want_l[0][i], 2 * abs(l32[i] - want_l[0][i]))
        assert abs(got[0][i] - want_l[0][i]) <= tol, (i, got[0][i], want_l[0][i], tol)
    for s in (1, 2):                                     # later steps: the same gate relative to the reference's own trajectory
        for i in range(2):
            tol = max(1e-5 * want_l[s][i], 2 * abs(l32[i] - want_l[0][i]) * want_l[s][i] / want_l[0][i])
            assert abs(got[s][i] - want_l[s][i]) <= tol, (s, i, got[s][i], want_l[s][i], tol)
    idx = f['idx'].astype(np.int64)
    g32 = flatten_state(g32, g32).astype(np.float64)
    bad = _sampled_gate(flatten_state(*g1).astype(np.float64), f['grad1'], idx, f['gmax'], g32)
    assert not bad, bad
    w3 = flatten_state(enc, dec).astype(np.float64)[idx] + f['dw3']
    d = np.abs(tr.flat_params().numpy().astype(np.float64)[idx] - w3)
    lr = float(f['lr'])
    assert d.max() <= 2 * lr * 3, d.max()
    assert (d > 0.01 * lr).mean() <= 1e-3, (d > 0.01 * lr).mean()
    tr.close()


@pytest.mark.timeout(300)
def test_float64_gradient_parity_bs4_full_shape():
    f, enc, dec = _fix()
    clip = torch.from_numpy(f['clip_img'])
    clip4 = torch.cat([clip, clip.flip(-1)])                  # the fixture's clips and the same motions played backwards
    x = network_input(clip4)
    tr = SmoothPriorTrainer(enc, dec, batch=4, H=245, W=135, lr=1e-4, device='cuda', use_graph=False)
    tr.step(x.cuda(), prepared=True)
    got = unflatten_state(tr.flat_grads().numpy())
    got = {**got[0], **got[1]}
    tr.close()
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    _, want = R.grads(enc, dec, x, dtype=torch.float64)
    floor = _fp32_floor(enc, dec, x, want)
    bad = R.per_tensor_gate(got, want, rel=2e-5, floor=floor)
    assert not bad, bad


@pytest.mark.timeout(600)
def test_bs60_graph_replay_and_two_engines_are_bit_identical_and_match_torch_fp32():
    enc, dec = R.random_state(11)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(60, 245, 135, generator=g) * 0.3).cuda()
    runs = {}
    for name, graph in (('graph', True), ('eager', False), ('graph2', True)):
        tr = SmoothPriorTrainer(enc, dec, batch=60, H=245, W=135, lr=1e-4, device='cuda', use_graph=graph)
        ls = [tr.step(x, prepared=True) for _ in range(20)]
        runs[name] = (ls, tr.flat_params())
        tr.close()
        del tr
        torch.cuda.empty_cache()
    for name in ('eager', 'graph2'):
        assert runs[name][0] == runs['graph'][0]
        assert torch.equal(runs[name][1], runs['graph'][1])
    assert all(np.isfinite(l).all() for l in runs['graph'][0])
    e = {k: v.cuda() for k, v in enc.items()}
    d = {k: v.cuda() for k, v in dec.items()}
    with torch.no_grad():
        _, lr_, ls, _, _ = R.forward_loss(e, d, x)
    l1 = runs['graph'][0][0]
    assert abs(l1[0] - float(lr_)) <= 1e-4 * float(lr_) and abs(l1[1] - float(ls)) <= 1e-4 * float(ls), (l1, float(lr_), float(ls))


def test_dec_module_reproduces_the_reference_on_15217():
    f, enc, dec = _fix()
    clip = torch.from_numpy(f['clip_img'])
    x = network_input(clip)[:1].cuda()
    E = priors.Enc(downsample=False, z_channel=64).cuda()
    E.load_state_dict(enc)
    D = priors.Dec(downsample=False, z_channel=64).cuda()
    D.load_state_dict(dec)
    with torch.no_grad():
        z, *sizes = E(x.unsqueeze(1))
        rec = D(z, *sizes)[0, 0].double().cpu()
    want = torch.from_numpy(f['dec_enc0'].astype(np.float64))
    assert float((rec - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_state_dict_round_trip_into_priors_enc(monkeypatch):
    enc, dec = R.random_state(21)
    g = torch.Generator().manual_seed(22)
    x = (torch.randn(1, 245, 135, generator=g) * 0.3).cuda()
    tr = SmoothPriorTrainer(enc, dec, batch=1, H=245, W=135, lr=1e-4, device='cuda')
    tr.step(x, prepared=True, n=2)
    _, sm = tr.evaluate(x, prepared=True)
    esd, dsd = tr.state_dicts()
    tr.close()
    monkeypatch.setattr(priors, 'DEFAULT_CONV_VARIANT', 2)        # the engine's kernels: conv3x3_mfma_lds
    E = priors.Enc(downsample=False, z_channel=64)
    E.load_state_dict(esd)
    D = priors.Dec(downsample=False, z_channel=64)
    D.load_state_dict(dsd)
    s2 = float(E.smooth_loss(x.unsqueeze(1)))
    assert abs(s2 - sm) <= 1e-6 * abs(sm), (s2, sm)
