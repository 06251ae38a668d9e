"""CPU suite: the infilling-prior training step (lemo_aetrain_*, csrc/ae_train_engine.hip) on the host emulator against a float64
restatement of models/AE.py + train_infill_prior.py:185-203 (tests/infill_train_common.py), at a small odd shape; the masking
helpers against literal restatements of the reference loops."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import infill_train_common as R
from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.infill_train import (InfillPriorTrainer, default_ae_state, flatten_state, load_prox_mask_clips, mask_prox,
                                   mask_random_markers, n_param, network_tensors, param_layout, unflatten_state)

BS, D, T = 3, 16, 9                      # network input 18 x 25
H, W = D + 2, T + 16
ERR_ARG, ERR_STATE = 10002, 10003


def _batch(seed, bs=BS):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(bs, 4, D, T, generator=g) * 0.5
    img[:, 0, -4:] = (torch.rand(bs, 4, T, generator=g) > 0.5).float()       # contact labels
    inp = img.clone()
    inp[:, 0, 3:9] = 0.
    return inp, img


def test_mask_random_markers_matches_the_reference_loop():
    d, T_ = 208, 7
    img = torch.randn(4, 4, d, T_)
    ids = torch.tensor([[16, 2, 5], [47, 1, 1], [30, 60, 66], [0, 3, 4]])
    want = img.clone().numpy()
    rows = ids.numpy() * 3 + 3
    for i in range(4):
        for r in (rows[i], rows[i] + 1, rows[i] + 2):
            want[i, 0, r, :] = 0.
        if 16 in ids[i] or 30 in ids[i]:
            want[i, 0, -4, :] = 0.
            want[i, 0, -2, :] = 0.
        if 47 in ids[i] or 60 in ids[i]:
            want[i, 0, -3, :] = 0.
            want[i, 0, -1, :] = 0.
    got = mask_random_markers(img, ids)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(img.numpy(), img.clone().numpy())                   # the input is not modified
    assert float(got[0, 0, -4].abs().sum()) == 0 and float(got[3, 0, -4].abs().sum()) != 0


def test_prox_masks_load_filter_and_apply(tmp_path):
    rng = np.random.default_rng(3)
    a = np.ones((250, 67), np.float32)
    a[:120, 16] = 0                          # clip 0: 120 / 8040 = 1.5 % masked -> dropped
    a[120:240, :10] = 0                      # clip 1: 15 % masked -> kept; frames 240.. are no whole clip
    b = (rng.random((120, 67)) > 0.3).astype(np.float32)
    for name, m in (('seqA', a), ('seqB', b)):
        os.makedirs(tmp_path / name)
        np.save(tmp_path / name / 'mask_markers.npy', m)
    clips = load_prox_mask_clips(str(tmp_path))
    assert clips.shape == (2, 120, 201)
    assert np.array_equal(clips[0], np.repeat(a[120:240], 3, axis=1)) and np.array_equal(clips[1], np.repeat(b, 3, axis=1))
    d, T_ = 208, 119
    img = torch.randn(2, 4, d, T_)
    got = mask_prox(img, clips).numpy()
    want = img.clone().numpy()
    for i in range(2):
        m = clips[i].T[:, :T_]                                                 # [201, T]
        left = (m[48] == 1) & (m[90] == 1)
        right = (m[141] == 1) & (m[180] == 1)
        full = np.concatenate([np.ones((3, T_)), m, np.stack([left, right, left, right]).astype(np.float64)])
        want[i, 0] = want[i, 0] * full.astype(np.float32)
    assert np.array_equal(got, want)


def test_default_state_is_deterministic_with_torch_bounds():
    a, b, c = default_ae_state(5), default_ae_state(5), default_ae_state(6)
    assert list(a) == [k for k, _ in param_layout()] and len(a) == 40
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a['enc_blc1.main.0.weight'], c['enc_blc1.main.0.weight'])
    assert sum(v.numel() for v in a.values()) == n_param()
    for k, v in a.items():
        fan_in = (a[k] if k.endswith('weight') else a[k[:-4] + 'weight']).shape[1] * 9
        assert float(v.abs().max()) <= 1 / np.sqrt(fan_in)
        assert float(v.abs().max()) > 0.9 / np.sqrt(fan_in) or v.numel() < 40
    assert a['dec_blc5.deconv1.weight'].shape == (32, 1, 3, 3) and float(a['dec_blc5.deconv1.weight'].abs().max()) > 0.3   # fan_in = 1 * 9: bound 1 / 3


def test_network_tensors_pad_like_the_reference():
    inp, img = _batch(1)
    x, y = network_tensors(inp, img)
    assert x.shape == (BS, 4, H, W) and y.shape == (BS, H, W)
    assert torch.equal(y[:, 1:-1, 8:-8], img[:, 0]) and torch.equal(y[:, 0], y[:, 2]) and torch.equal(y[:, :, 7], y[:, :, 9])


def test_evaluate_matches_float64(emu_lib):
    sd = default_ae_state(2)
    inp, img = _batch(3)
    tr = InfillPriorTrainer(sd, batch=BS, H=H, W=W, lr=1e-3, _lib=emu_lib)
    *got, rec = tr.evaluate(inp, img, return_rec=True)
    x, y = network_tensors(inp, img)
    want, _ = R.step(sd, x, y)
    wrec = R.ae_forward({k: v.double() for k, v in sd.items()}, x.double())
    assert rec.shape == (BS, 1, H, W)
    assert float((rec.double() - wrec).abs().max()) < 1e-5 * float(wrec.abs().max())
    for k in range(3):
        assert abs(got[k] - want[k]) < 1e-5 * abs(want[k]), (k, got[k], want[k])
    assert abs(tr.last_total() - want[3]) < 1e-5 * want[3]
    # a target equal to the reconstruction has zero L1 and velocity terms
    y2 = rec[:, 0].clone()
    l2 = tr.evaluate(x, y2, prepared=True)
    assert l2[0] == 0.0 and l2[1] == 0.0
    tr.close()


def test_exact_ties_take_sign_zero_in_the_adjoint(emu_lib):
    """rec == y exactly at many pixels (the last layer's weights zero: rec = its bias in every dtype): the L1 and velocity adjoints
    must use sign(0) = 0 there, as torch's L1 backward does; sign(0) = +-1 would move the last layer's gradients"""
    sd = default_ae_state(9)
    sd['dec_blc5.deconv2.weight'] = torch.zeros(1, 1, 3, 3)
    sd['dec_blc5.deconv2.bias'] = torch.full((1,), 0.375)
    inp, img = _batch(10)
    x, y = network_tensors(inp, img)
    tie = torch.rand(y.shape, generator=torch.Generator().manual_seed(11)) < 0.5
    y = torch.where(tie, torch.full_like(y, 0.375), y).contiguous()
    tr = InfillPriorTrainer(sd, batch=BS, H=H, W=W, lr=1e-3, _lib=emu_lib)
    tr.step(x, y, prepared=True)
    _, want_g = R.step(sd, x, y)
    got_g = unflatten_state(tr.flat_grads())
    assert float(want_g['dec_blc5.deconv2.bias'].abs()) > 0
    assert not R.per_tensor_gate(got_g, want_g, rel=2e-5), R.per_tensor_gate(got_g, want_g, rel=2e-5)
    tr.close()


@pytest.mark.parametrize('logit', [100.0, -100.0])
def test_large_logits_stay_finite(emu_lib, logit):
    """the BCE term evaluated as torch does: logits of +-100 give finite losses and gradients"""
    sd = default_ae_state(4)
    sd['dec_blc5.deconv2.bias'] = torch.full((1,), logit)
    inp, img = _batch(5)
    x, y = network_tensors(inp, img)
    tr = InfillPriorTrainer(sd, batch=BS, H=H, W=W, lr=1e-3, _lib=emu_lib)
    got = tr.step(x, y, prepared=True)
    want, want_g = R.step(sd, x, y)
    assert all(np.isfinite(got)) and all(abs(got[k] - want[k]) < 1e-5 * abs(want[k]) for k in range(3)), (got, want)
    g = unflatten_state(tr.flat_grads())
    assert torch.isfinite(R.flat(g)).all()
    assert not R.per_tensor_gate(g, want_g, rel=2e-5), R.per_tensor_gate(g, want_g, rel=2e-5)
    tr.close()


def test_two_engine_steps_match_float64(emu_lib):
    sd = default_ae_state(7)
    inp, img = _batch(8)
    x, y = network_tensors(inp, img)
    lr = 1e-3
    tr = InfillPriorTrainer(sd, batch=BS, H=H, W=W, lr=lr, _lib=emu_lib)
    s1 = tr.step(inp, img)
    want1, want_g = R.step(sd, x, y)
    assert all(abs(s1[k] - want1[k]) < 1e-5 * abs(want1[k]) for k in range(3)), (s1, want1)
    got_g = unflatten_state(tr.flat_grads())
    assert not R.per_tensor_gate(got_g, want_g, rel=2e-5), R.per_tensor_gate(got_g, want_g, rel=2e-5)
    s2 = tr.step(inp, img)
    hist, want_p = R.train(sd, x, y, 2, lr)
    assert all(abs(s2[k] - hist[1][k]) < 1e-5 * abs(hist[1][k]) for k in range(3)), (s2, hist[1])
    assert R.sign_flip_gate(tr.state_dict(), want_p, lr, 2)
    tr.close()


@pytest.mark.parametrize('bs', [1, 9])
def test_weight_gradient_sums_over_every_batch_size(emu_lib, bs):
    """bs = 1 (one image group) and bs = 9 (more images than weight-gradient groups, unequal groups): every gradient entry"""
    sd = default_ae_state(11)
    inp, img = _batch(12, bs=bs)
    tr = InfillPriorTrainer(sd, batch=bs, H=H, W=W, lr=1e-4, _lib=emu_lib)
    tr.step(inp, img)
    _, want_g = R.step(sd, *network_tensors(inp, img))
    got_g = unflatten_state(tr.flat_grads())
    assert not R.per_tensor_gate(got_g, want_g, rel=2e-5), R.per_tensor_gate(got_g, want_g, rel=2e-5)
    tr.close()


def test_pool_winners_are_the_maxima_of_the_encoder_activations(emu_lib):
    """lemo_aetrain_pool_winners: forcing them on the float64 restatement gives the free float64 forward wherever the two agree"""
    sd = default_ae_state(14)
    inp, img = _batch(15)
    tr = InfillPriorTrainer(sd, batch=BS, H=H, W=W, lr=1e-4, _lib=emu_lib)
    tr.evaluate(inp, img)
    win = tr.pool_winners()
    assert [tuple(w.shape) for w in win] == [(BS, 32, 9, 13), (BS, 64, 5, 7), (BS, 128, 3, 4), (BS, 256, 2, 2), (BS, 256, 1, 1)]
    assert all(int(w.max()) <= 8 for w in win)
    x, y = network_tensors(inp, img)
    p = {k: v.double() for k, v in sd.items()}
    free, forced = R.ae_forward(p, x.double()), R.ae_forward(p, x.double(), win)
    assert float((free - forced).abs().max()) < 1e-12
    tr.close()


def test_load_resets_and_params_round_trip(emu_lib):
    sd = default_ae_state(13)
    tr = InfillPriorTrainer(sd, batch=1, H=H, W=W, lr=1e-4, _lib=emu_lib)
    got = tr.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert torch.equal(torch.from_numpy(flatten_state(got)), tr.flat_params())
    tr.close()


def test_wrong_inputs_raise(emu_lib):
    tr = InfillPriorTrainer(None, batch=2, H=H, W=W, _lib=emu_lib)
    inp, img = _batch(1, bs=2)
    with pytest.raises(ValueError):
        tr.step(inp[:1], img[:1])                       # wrong batch size
    with pytest.raises(ValueError):
        tr.step(inp[:, :, :-1], img[:, :, :-1])         # wrong clip shape
    with pytest.raises(ValueError):
        tr.step(inp[:, :1], img[:, :1])                 # 1-channel body mode
    with pytest.raises(TypeError):
        tr.step(inp.numpy(), img)
    tr.close()
    for bad in [dict(batch=0), dict(batch=129), dict(H=5), dict(W=1)]:
        kw = dict(batch=2, H=H, W=W)
        kw.update(bad)
        with pytest.raises(ValueError):
            InfillPriorTrainer(None, _lib=emu_lib, **kw)


def test_engine_argument_and_state_errors(emu_lib):
    lib = emu_lib
    assert lib.aetrain_ws_floats(H, W, 0) == 0 and lib.aetrain_ws_floats(H, W, 129) == 0 and lib.aetrain_ws_floats(5, W, 1) == 0
    n1, n2 = lib.aetrain_ws_floats(H, W, 1), lib.aetrain_ws_floats(H, W, 2)
    assert 0 < n1 < n2
    ws = torch.zeros(int(n1))
    d = _hip.AetrainDesc(H=H, W=W, bs=1, lr=1e-4, w_body=10., w_v=10., w_c=1., ws=ptr(ws), ws_floats=int(n1) - 1, use_graph=0)
    assert not lib.aetrain_create(C.byref(d))                                    # workspace too small
    d.ws_floats = int(n1)
    d.lr = 0.0
    assert not lib.aetrain_create(C.byref(d))                                    # lr must be positive
    d.lr = 1e-4
    h = lib.aetrain_create(C.byref(d))
    assert h
    x, y, out = torch.zeros(4, H, W), torch.zeros(H, W), torch.zeros(n_param())
    try:
        assert lib.aetrain_step(h, ptr(x), ptr(y), 1, None, None) == ERR_STATE
        assert lib.aetrain_eval(h, ptr(x), ptr(y), ptr(out), None, None) == ERR_STATE
        assert lib.aetrain_params(h, ptr(out), None) == ERR_STATE
        assert lib.aetrain_grads(h, ptr(out), None) == ERR_STATE
        assert lib.aetrain_step(h, None, ptr(y), 1, None, None) == ERR_ARG
        assert lib.aetrain_step(h, ptr(x), ptr(y), -1, None, None) == ERR_ARG
        assert lib.aetrain_step(h, ptr(x), ptr(y), 0, None, None) == ERR_ARG
        assert lib.aetrain_pool_winners(h, 0, ptr(out), None) == ERR_STATE
        assert lib.aetrain_load(h, None, None) == ERR_ARG
    finally:
        lib.aetrain_destroy(h)
    assert n_param() == lib.ae_n_param()


def test_aetrain_descriptor_layout_matches_the_header():
    """the ctypes mirror of lemo_aetrain_desc has the C struct's size and field offsets (compiled from include/lemo_hip.h)"""
    fl = ['W', 'bs', 'lr', 'w_body', 'w_v', 'w_c', 'ws', 'ws_floats', 'use_graph']
    src = '#include <cstdio>\n#include <cstddef>\n#include "lemo_hip.h"\nint main(){\n'
    src += 'printf("%zu", sizeof(lemo_aetrain_desc));' + ''.join(f'printf(" %zu", offsetof(lemo_aetrain_desc, {f}));' for f in fl)
    src += 'printf("\\n"); return 0;}\n'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, 'o.cpp'), 'w').write(src)
        subprocess.run(['g++', '-I', os.path.join(root, 'include'), os.path.join(td, 'o.cpp'), '-o', os.path.join(td, 'o')], check=True)
        line = subprocess.run([os.path.join(td, 'o')], check=True, capture_output=True, text=True).stdout.strip()
    want = [int(v) for v in line.split()]
    got = [C.sizeof(_hip.AetrainDesc)] + [getattr(_hip.AetrainDesc, f).offset for f in fl]
    assert got == want


def test_new_kernels_use_no_scratch_and_fit_their_register_budget():
    """ae_train_engine.hip's kernels: no scratch; the weight-gradient wave keeps ae_wgrad_multi_kernel's 128-register budget"""
    from test_resource_usage import _usage
    res = _usage('ae_train_engine.hip')
    names = [k for k in res if 'aet_' in k]
    assert len(names) >= 6, names
    for k in names:
        assert res[k].get('ScratchSize [bytes/lane]', 0) == 0, k
        assert res[k].get('VGPRs Spill', 0) == 0, k
    wg = [k for k in names if 'aet_wgrad_kernel' in k]
    assert wg and res[wg[0]]['VGPRs'] <= 128
