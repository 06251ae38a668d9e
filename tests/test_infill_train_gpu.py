"""GPU suite: the infilling-prior training engine (lemo_aetrain_*) on an MI355X at the shipped shape (210 x 135): every gradient
entry against float64 on the engine's max-pool branch, determinism at bs = 60 / 120 (graph replay, eager, a second engine), losses against torch
fp32 autograd, and the round trip of the trained state_dict into lemo_amd.infill.AE and the finetune engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import infill_train_common as R
from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.infill import AE
from lemo_amd.infill_train import InfillPriorTrainer, default_ae_state, flatten_state, mask_random_markers, network_tensors, unflatten_state

pytestmark = pytest.mark.gpu
D, T = 208, 119
H, W = D + 2, T + 16


def _batch(seed, bs, dev='cuda'):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(bs, 4, D, T, generator=g) * 0.5
    img[:, 0, -4:] = (torch.rand(bs, 4, T, generator=g) > 0.5).float()
    ids = (torch.rand(bs, 4, generator=g) * 67).long()
    ids[0, 0] = 16
    inp = mask_random_markers(img, ids)
    return inp.to(dev), img.to(dev)


def _enc_acts(sd, x):
    """float64 outputs of the five encoder blocks' second layers (what each max pool reads)"""
    import torch.nn.functional as F
    h, out = x.double(), []
    p = {k: v.double() for k, v in sd.items()}
    for b in range(1, 6):
        k = f'enc_blc{b}.main.'
        h = F.leaky_relu(F.conv2d(h, p[k + '0.weight'], p[k + '0.bias'], padding=1), 0.2)
        h = F.leaky_relu(F.conv2d(h, p[k + '2.weight'], p[k + '2.bias'], padding=1), 0.2)
        out.append(h)
        h = F.max_pool2d(h, 3, 2, 1)
    return out


def test_every_gradient_entry_matches_float64_at_bs4():
    """bs = 4 at 210 x 135 from torch's default init.  Max pooling is discontinuous: where two entries of a window are within fp32
    rounding of each other, fp32 and float64 can pick different winners, and the whole gradient behind that window moves.  So:
    (1) every window whose engine winner is not float64's winner must be such a near-tie, and (2) with the engine's winners the
    float64 gradient must match every engine gradient entry within 2e-5 x max |g| per tensor."""
    sd = default_ae_state(21)
    inp, img = _batch(22, 4)
    tr = InfillPriorTrainer(sd, batch=4, H=H, W=W, lr=1e-4)
    got = tr.step(inp, img)
    win = tr.pool_winners()
    x, y = network_tensors(inp.cpu(), img.cpu())
    for b, a in enumerate(_enc_acts(sd, x)):
        v64, i64 = torch.nn.functional.max_pool2d(a, 3, 2, 1, return_indices=True)
        from lemo_amd.infill_torch import _pool
        ve = _pool(a, win[b])
        gap = (v64 - ve)                                                      # >= 0; 0 where the winners agree
        assert float(gap.min()) >= 0
        assert float(gap.max()) <= 2e-6 * float(a.abs().max()), (b, float(gap.max()), float(a.abs().max()))
    want, want_g = R.step(sd, x, y, winners=win)
    assert all(abs(got[k] - want[k]) < 1e-5 * abs(want[k]) for k in range(3)), (got, want)
    g = unflatten_state(tr.flat_grads())
    bad = R.per_tensor_gate(g, want_g, rel=2e-5)
    assert not bad, bad
    tr.close()


@pytest.mark.parametrize('bs', [60, 120])
def test_replay_eager_and_second_engine_are_bit_identical_and_match_torch(bs):
    sd = default_ae_state(31)
    inp, img = _batch(32 + bs, bs)
    steps, lr = 10, 1e-4
    a = InfillPriorTrainer(sd, batch=bs, H=H, W=W, lr=lr, use_graph=True)
    la = [a.step(inp, img) + (a.last_total(),) for _ in range(steps)]
    pa = a.flat_params()
    a.close()
    b = InfillPriorTrainer(sd, batch=bs, H=H, W=W, lr=lr, use_graph=False)
    lb = [b.step(inp, img) + (b.last_total(),) for _ in range(steps)]
    pb = b.flat_params()
    b.close()
    c = InfillPriorTrainer(sd, batch=bs, H=H, W=W, lr=lr, use_graph=True)
    c.step(inp, img, n=steps)
    pc = c.flat_params()
    c.close()
    assert la == lb and torch.equal(pa, pb) and torch.equal(pa, pc)
    x, y = network_tensors(inp, img)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    hist, _ = R.train({k: v.cuda() for k, v in sd.items()}, x, y, steps, lr, dtype=torch.float32)
    for s in range(steps):
        for k in range(4):
            assert abs(la[s][k] - hist[s][k]) <= 2e-4 * abs(hist[s][k]), (s, k, la[s][k], hist[s][k])


def test_state_dict_round_trip_into_the_module_and_the_finetune_engine():
    inp, img = _batch(41, 2)
    tr = InfillPriorTrainer(None, batch=2, H=H, W=W, lr=1e-3, seed=3)
    tr.step(inp, img, n=3)
    *_, rec = tr.evaluate(inp, img, return_rec=True)
    sd = tr.state_dict()
    assert all(v.device.type == 'cpu' for v in sd.values())
    m = AE().cuda()
    m.load_state_dict(sd)
    x, _ = network_tensors(inp, img)
    with torch.no_grad():
        for i in range(2):
            out, _ = m(x[i:i + 1])
            assert float((out[0, 0] - rec[i, 0]).abs().max()) <= 1e-5 * float(rec[i].abs().max())
    lib = _hip.get_lib()
    n = int(lib.ae_ws_floats(H, W))
    ws = torch.zeros(n, device='cuda')
    h = lib.ae_create(C.byref(_hip.AeDesc(H, W, 3e-6, ptr(ws), n, 1)))
    assert h
    flat = torch.from_numpy(flatten_state(sd)).cuda()
    moc = torch.ones(H, W, device='cuda') / (H * W)
    r2 = torch.zeros(H, W, device='cuda')
    xc = x[0].contiguous()
    assert lib.ae_load(h, ptr(flat), ptr(xc), ptr(moc), None) == 0
    assert lib.ae_forward(h, ptr(r2), None, None) == 0
    torch.cuda.synchronize()
    assert float((r2 - rec[0, 0]).abs().max()) <= 1e-5 * float(rec[0].abs().max())
    lib.ae_destroy(h)
    tr.close()


def test_cpu_tensors_and_wrong_batches_raise():
    tr = InfillPriorTrainer(None, batch=2, H=H, W=W)
    inp, img = _batch(1, 2)
    with pytest.raises(ValueError):
        tr.step(inp.cpu(), img.cpu())
    with pytest.raises(ValueError):
        tr.step(inp[:1], img[:1])
    tr.close()


def test_fixture_parity_with_the_reference_training_step():
    """tests/golden/infill_train.npz: the reference's own models/AE.py and loss in float64, 3 Adam steps at lr 1e-4 from
    default_ae_state(1234).  Losses within 1e-5 (relative) or 2 x torch fp32's distance; 3-step parameters inside the Adam sign-flip
    gate.  Step-1 gradients: the float64 restatement reproduces the fixture's (it IS the reference's function), and the engine
    matches the restatement on the engine's max-pool branch within 2e-5 x max |g| or 2 x torch fp32's distance, its winners
    differing from float64's only at near-ties (see test_every_gradient_entry_matches_float64_at_bs4)."""
    import os
    from lemo_amd.infill_train import n_param, param_layout
    f = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'infill_train.npz'))
    sd = default_ae_state(1234)
    assert np.allclose([float(sd[k].double().sum()) for k, _ in param_layout()], f['init_sums'], rtol=0, atol=1e-9)
    img = torch.from_numpy(f['clip_img'].astype(np.float32)).cuda()
    inp = torch.from_numpy(f['clip_img_input'].astype(np.float32)).cuda()
    lr, idx = float(f['lr']), torch.from_numpy(f['idx'].astype(np.int64))
    x, y = network_tensors(inp, img)
    hist32, _ = R.train({k: v.cuda() for k, v in sd.items()}, x, y, 3, lr, dtype=torch.float32)
    _, g32 = R.step({k: v.cuda() for k, v in sd.items()}, x, y, dtype=torch.float32)
    tr = InfillPriorTrainer(sd, batch=2, H=H, W=W, lr=lr)
    got, g1 = [], None
    for s in range(3):
        got.append(list(tr.step(inp, img)) + [tr.last_total()])
        if s == 0:
            g1 = tr.flat_grads().double()
            win = tr.pool_winners()
    want = f['losses']
    for s in range(3):
        for k in range(4):
            tol = max(1e-5 * abs(want[s][k]), 2 * abs(hist32[s][k] - want[s][k]))
            assert abs(got[s][k] - want[s][k]) <= tol, (s, k, got[s][k], want[s][k])
    _, g64 = R.step(sd, x.cpu(), y.cpu())
    _, g64w = R.step(sd, x.cpu(), y.cpu(), winners=win)
    g64f, g64wf, g32f = R.flat(g64), R.flat(g64w), R.flat(g32)
    o, bad = 0, []
    starts = {}
    for k, shp in param_layout():
        starts[k] = (o, o + int(np.prod(shp)))
        o += int(np.prod(shp))
    assert o == n_param()
    want_g = torch.from_numpy(f['grad1'])
    for t, (k, _) in enumerate(param_layout()):
        a, b = starts[k]
        sel = (idx >= a) & (idx < b)
        assert float((g64f[idx[sel]] - want_g[sel]).abs().max()) <= 1e-9 * float(f['gmax'][t]), k
        e = float((g1[idx[sel]] - g64wf[idx[sel]]).abs().max())
        e32 = float((g32f[idx[sel]] - want_g[sel]).abs().max())
        if e > max(2e-5 * float(f['gmax'][t]), 2 * e32):
            bad.append((k, e, 2e-5 * float(f['gmax'][t]), 2 * e32))
    assert not bad, bad
    dw = (R.flat(tr.state_dict()) - R.flat(sd))[idx] - torch.from_numpy(f['dw3'])
    assert float(dw.abs().max()) <= 2 * lr * 3 and float((dw.abs() > 0.01 * lr).double().mean()) <= 1e-3
    tr.close()
