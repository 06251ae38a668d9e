"""CPU suite: the smoothness-prior training step (lemo_sptrain_*, csrc/prior_train_*.hip) on the host emulator against a
float64 restatement of train_smooth_prior.py:96-136 (tests/sptrain_common.py), at a small odd shape."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sptrain_common as R
from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.priors import Dec, to_cg8p
from lemo_amd.smooth_train import SmoothPriorTrainer, flatten_state, n_param, param_layout, unflatten_state

BS, H, W = 3, 13, 20
ERR_SHAPE, ERR_ARG, ERR_STATE = 10001, 10002, 10003         # include/lemo_hip.h


def _x(seed, bs=BS):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(bs, H, W, generator=g) * 0.5


def _wgrad(lib, A, B, ca, cb, bias_b):
    """A [bs, ca, H, W], B [bs, cb, H, W] float32 -> (gw [ca][cb][3][3], gb) through lemo_wgrad3x3_batched"""
    bs = A.shape[0]
    pack = lambda T, c: (torch.stack([to_cg8p(T[b]) for b in range(bs)]) if c > 1 else F.pad(T[:, 0], (1, 1, 1, 1))).contiguous()
    Ap, Bp = pack(A, ca), pack(B, cb)
    ws = torch.zeros(int(lib.wgrad3x3_batched_ws_floats(H, W, bs, ca, cb)))
    gw = torch.zeros(ca, cb, 3, 3)
    gb = torch.zeros(cb if bias_b else ca)
    lib.check(lib.wgrad3x3_batched(ptr(Ap), Ap[0].numel(), ptr(Bp), Bp[0].numel(), bs, H, W, ca, cb, bias_b, ptr(ws), ptr(gw), ptr(gb), None),
              'wgrad3x3_batched')
    return gw, gb


@pytest.mark.parametrize('ca,cb', [(32, 32), (64, 32), (64, 64), (32, 1), (1, 1)])
def test_batched_weight_gradient_matches_float64(emu_lib, ca, cb):
    g = torch.Generator().manual_seed(ca * 100 + cb)
    A = torch.randn(BS, ca, H, W, generator=g)
    B = torch.randn(BS, cb, H, W, generator=g)
    Bd = F.pad(B.double(), (1, 1, 1, 1))
    want = torch.zeros(ca, cb, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            want[:, :, ky, kx] = torch.einsum('bmyx,bnyx->mn', A.double(), Bd[:, :, ky:ky + H, kx:kx + W])
    for bias_b in (0, 1):
        gw, gb = _wgrad(emu_lib, A, B, ca, cb, bias_b)
        assert float((gw.double() - want).abs().max()) < 2e-5 * float(want.abs().max())
        wb = (B if bias_b else A).double().sum((0, 2, 3))
        assert float((gb.double() - wb).abs().max()) < 1e-4 * float(wb.abs().max() + 1)


def test_weight_gradient_refuses_shapes_it_does_not_take(emu_lib):
    lib = emu_lib
    buf = torch.zeros(1 << 16)
    for ca, cb in [(16, 32), (32, 2), (64, 1), (2, 1)]:
        assert lib.wgrad3x3_batched(ptr(buf), 0, ptr(buf), 0, 1, 4, 4, ca, cb, 0, ptr(buf), ptr(buf), ptr(buf), None) == ERR_SHAPE
    assert lib.wgrad3x3_batched(ptr(buf), 0, ptr(buf), 0, 1, 4, 200, 64, 64, 0, ptr(buf), ptr(buf), ptr(buf), None) == ERR_SHAPE
    assert lib.wgrad3x3_batched(None, 0, ptr(buf), 0, 1, 4, 4, 32, 32, 0, ptr(buf), ptr(buf), ptr(buf), None) == ERR_ARG


def test_dec_module_matches_conv_transpose2d(emu_lib):
    enc, dec = R.random_state(3)
    m = Dec(downsample=False, z_channel=64, _lib=emu_lib)
    assert set(m.state_dict().keys()) == set(dec.keys())
    m.load_state_dict(dec)
    z = torch.randn(2, 64, H, W, generator=torch.Generator().manual_seed(4)).abs() * 0.3
    rec = m(z, None, None, None, None, None)
    h = z.double()
    for j in range(10):
        k = f'dec_blc{j // 2 + 1}.deconv{j % 2 + 1}'
        h = F.conv_transpose2d(h, dec[k + '.weight'].double(), dec[k + '.bias'].double(), stride=1, padding=1)
        if j != 9:
            h = F.leaky_relu(h, 0.2)
    assert rec.shape == (2, 1, H, W)
    assert float((rec.double() - h).abs().max()) < 1e-5 * float(h.abs().max())
    with pytest.raises(NotImplementedError):
        Dec(downsample=True)


def test_flat_layout_round_trips_and_counts_the_reference_parameters(emu_lib):
    enc, dec = R.random_state(5)
    assert n_param() == 536139 == emu_lib.sptrain_n_param()
    e2, d2 = unflatten_state(flatten_state(enc, dec))
    assert all(torch.equal(e2[k], enc[k]) for k in enc) and all(torch.equal(d2[k], dec[k]) for k in dec)


@pytest.mark.timeout(900)
def test_two_engine_steps_match_float64_training(emu_lib):
    enc, dec = R.random_state(7)
    x = _x(8)
    lr = 1e-3
    tr = SmoothPriorTrainer(enc, dec, batch=BS, H=H, W=W, lr=lr, _lib=emu_lib)
    l0 = tr.evaluate(x, prepared=True)
    (wl_rec, wl_sm), want_g = R.grads(enc, dec, x)
    assert abs(l0[0] - wl_rec) < 1e-5 * wl_rec and abs(l0[1] - wl_sm) < 1e-5 * wl_sm
    s1 = tr.step(x, prepared=True)
    assert abs(s1[0] - wl_rec) < 1e-5 * wl_rec and abs(s1[1] - wl_sm) < 1e-5 * wl_sm
    got_g = unflatten_state(tr.flat_grads().numpy())
    got_g = {**got_g[0], **got_g[1]}
    assert not R.per_tensor_gate(got_g, want_g, rel=2e-5), R.per_tensor_gate(got_g, want_g, rel=2e-5)
    s2 = tr.step(x, prepared=True)
    losses, want_p = R.train(enc, dec, x, 2, lr=lr)
    assert abs(s2[0] - losses[1][0]) < 1e-5 * losses[1][0] and abs(s2[1] - losses[1][1]) < 1e-5 * losses[1][1]
    enc2, dec2 = tr.state_dicts()
    got_p = R.flat({**enc2, **dec2})
    d = (got_p - R.flat(want_p)).abs()
    assert float(d.max()) <= 2 * lr * 2
    assert float((d > 0.01 * lr).double().mean()) <= 1e-3
    tr.close()


def test_engine_argument_and_state_errors(emu_lib):
    lib = emu_lib
    assert lib.sptrain_ws_floats(H, 140, 1) == 0 and lib.sptrain_ws_floats(1, W, 1) == 0 and lib.sptrain_ws_floats(H, W, 0) == 0
    n = lib.sptrain_ws_floats(H, W, 1)
    ws = torch.zeros(int(n))
    d = _hip.SptrainDesc(H=H, W=W, bs=1, lr=1e-4, weight_rec=1.0, weight_smooth=1000.0, ws=ptr(ws), ws_floats=int(n) - 1, use_graph=0)
    assert not lib.sptrain_create(C.byref(d))                                    # workspace too small
    d.ws_floats = int(n)
    h = lib.sptrain_create(C.byref(d))
    assert h
    x = torch.zeros(H, W)
    out = torch.zeros(n_param())
    try:
        assert lib.sptrain_step(h, ptr(x), 1, None, None) == ERR_STATE
        assert lib.sptrain_eval(h, ptr(x), ptr(out), None, None) == ERR_STATE
        assert lib.sptrain_params(h, ptr(out), None) == ERR_STATE
        assert lib.sptrain_step(h, None, 1, None, None) == ERR_ARG
        assert lib.sptrain_load(h, None, None) == ERR_ARG
    finally:
        lib.sptrain_destroy(h)


def test_sptrain_descriptor_layout_matches_the_header():
    """the ctypes mirror of lemo_sptrain_desc has the C struct's size and field offsets (compiled from include/lemo_hip.h)"""
    fl = ['W', 'bs', 'lr', 'weight_rec', 'weight_smooth', 'ws', 'ws_floats', 'use_graph']
    src = '#include <cstdio>\n#include <cstddef>\n#include "lemo_hip.h"\nint main(){\n'
    src += 'printf("%zu", sizeof(lemo_sptrain_desc));' + ''.join(f'printf(" %zu", offsetof(lemo_sptrain_desc, {f}));' for f in fl)
    src += 'printf("\\n"); return 0;}\n'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, 'o.cpp'), 'w').write(src)
        subprocess.run(['g++', '-I', os.path.join(root, 'include'), os.path.join(td, 'o.cpp'), '-o', os.path.join(td, 'o')], check=True)
        line = subprocess.run([os.path.join(td, 'o')], check=True, capture_output=True, text=True).stdout.strip()
    want = [int(v) for v in line.split()]
    got = [C.sizeof(_hip.SptrainDesc)] + [getattr(_hip.SptrainDesc, f).offset for f in fl]
    assert got == want
