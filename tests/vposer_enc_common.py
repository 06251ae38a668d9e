"""Direct tests of the VPoser encoder (csrc/vposer_enc_kernels.hip) through its two C entry points and through the Python surface built
on them, against float64 on the CPU (tests/test_vposer_enc_emu.py on the host-emulated build, tests/test_vposer_enc_gpu.py on the
MI355X; both run the cases below):

  lemo_vposer_encode_fwd / _bwd       eval-mode encoder and its input gradient, one launch each
  VPoser.encode / forward / sample_poses / matrot2aa / aa2matrot, embed_body_pose             lemo_amd/vposer.py
  with_pose_embedding                                                                          lemo_amd/prox_windows.py

Reference arithmetic: `restate` below, vposer_smpl.py:98-105 in eval mode and UNFOLDED -- F.batch_norm with the running statistics and
eps 1e-5, then the layer -- in float64 from the same float32 parameters and inputs.  The yardstick is the same function in float32 torch
on the CPU.  Never another kernel form, never torch on the GPU.  Parameters come from make_vposer_enc_weights (BatchNorm terms far from
the identity); inputs are axis-angle vectors of sigma 0.4.

Tolerances
----------
err(v) = max |v - ref| / max |ref| per output tensor; blocks_common.gate as it stands: GATE = 4 x the float32 restatement's own distance
from float64, floor 2^-23 where that is zero.  On top of it, ONE derived term (lbs_common.gate_plus adds it to the bound):
* The library folds bn1 into fc1 and bn2 into fc2 in float64 and rounds every folded weight and bias once to float32
  (lemo_amd.vposer.fold_vposer_enc).  With u = 2^-24 a folded weight is W' (1 + d), |d| <= u, so a pre-activation of layer 1 is off by at
  most E1 = u (sum_k |W1'_mk| |x_k| + |b1'_m|), and so is h1 (LeakyReLU has slope <= 1).  Layer 2 adds its own roundings and carries E1
  on: E2 = u (sum_k |W2'_mk| |h1_k| + |b2'_m|) + sum_k |W2'_mk| E1_k.  The head is not folded; it carries E2 on:
  E(mean_j) = sum_k |Wmu_jk| E2_k, E(lv_j) likewise with logvar, and E(std) = E(lv) (softplus has slope <= 1).  `fold_terms` evaluates
  these first-order bounds in float64 for the case's own inputs; max E / max |ref| is the term.
* Backward, the same roundings: d(h2) = head^T d(head) uses no folded weight.  With d2 = d(h2) lrelu'(h2), d(h1) = W2'^T d2 is off by at
  most F1 = u sum_m |W2'_mk| |d2_m|, and d(x) = W1'^T d1 by at most u sum_m |W1'_mc| |d1_m| + sum_m |W1'_mc| F1_m (`fold_terms_bwd`).
* No split-f16 form ships, so there is no 2^-21 term.
* Backward inputs: the test SUPPLIES h1, h2 and lv -- the float64 forward rounded to float32.  Rounding keeps every sign, so both
  LeakyReLU decisions are inputs of the kernel and of the reference alike (checked on the host: no supplied h is 0), and the softplus
  derivative is evaluated by both from the same float32 lv.  The reference is autograd of `restate` with those decisions.
* Bit checks (no rounding freedom): h1 = h2 = lv = NULL against the saving call; a NULL gradient against a zero tensor; encode on the
  three input shapes, autograd through VPoser.encode, forward(eps) and sample_poses against the C entries / decode on the same numbers.
* pose_aa of forward(eps) against the reference's recorded run: the gate with the float32 restatement of encode -> sample -> decode as
  yardstick, plus the decoder's existing tolerance of the vposer-decode golden test (1e-4 relative, tests/test_gpu_parity.py VERT_TOL,
  tests/test_kernels_emu.py): that part is the shipped decoder.
* aa2matrot(matrot2aa(R)) == R within 2^-20 absolute: existing rotation helpers, checks wiring and shapes only.  The rotations are
  axis-angle vectors of sigma 0.4 per component, the range of the encoder's own inputs.

Buffers: as in lbs_common -- every output between GUARD sentinels and pre-filled with NaN; the 63-float input rows are packed so that the
float after the last row is a guard (NaN: reading element 63 of the last row would poison the result); in the strided case (pin_stride 165,
out_stride 56, the input 3 floats into its row like the body pose inside a full pose) every column the kernel must not read holds NaN and
every column it must not write must still hold NaN afterwards.  A refused call leaves every output NaN."""
import ctypes as C
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from blocks_common import ERR_ARG, NAN, RATIOS, U, _sync, gate, guarded, guards_intact, same_bits
from lbs_common import gate_plus
from lemo_amd._hip import ptr
from lemo_amd.vposer import (BN_EPS, VPoser, embed_body_pose, fold_vposer_enc, make_vposer_enc_weights, make_vposer_weights,
                             vposer_enc_weight_struct)

LAUNCHED = set()                  # 'fwd' / 'bwd': what the checks of this process launched
SIGMA = 0.4
FWD_B = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 119, 257)      # one row; every side of a 16-, 32- and 64-row tile; several workgroups, ragged tail
FWD_CASES = [(B, 'plain') for B in FWD_B] + [(33, 'softplus'), (65, 'strided'), (17, 'nosave')]
BWD_CASES = [(1, 'both', 'plain'), (17, 'mean', 'plain'), (33, 'std', 'softplus'), (119, 'both', 'plain'), (17, 'std', 'plain'),
             (33, 'both', 'strided')]                          # (B, gradients given, variant)
LARGE_B = 65537
LV_SCALE = 48.0                   # 'softplus' / 'strided' variants: logvar head scaled so that lv leaves [-20, 20] on both sides


# ---------------------------------------------------------------------------------------------------------------------------
# parameters, inputs and the restatement

@functools.lru_cache(maxsize=None)
def enc_state(seed=2, lv_scale=1.0, var_scale=1.0):
    """float32 numpy state of the encoder; lv_scale multiplies the logvar head, var_scale bn1's running variance"""
    w = make_vposer_enc_weights(seed)
    if lv_scale != 1.0:
        for k in ('weight', 'bias'):
            w['bodyprior_enc_logvar.' + k] = (w['bodyprior_enc_logvar.' + k] * np.float32(lv_scale)).astype(np.float32)
    if var_scale != 1.0:
        w['bodyprior_enc_bn1.running_var'] = (w['bodyprior_enc_bn1.running_var'] * np.float32(var_scale)).astype(np.float32)
    return w


def variant_state(variant):
    return enc_state(2, LV_SCALE if variant in ('softplus', 'strided') else 1.0)


def poses(B, seed):
    return torch.randn(B, 63, generator=torch.Generator().manual_seed(seed)) * SIGMA


def restate(sd, x, dtype, decisions=None):
    """vposer_smpl.py:98-105 in eval mode, unfolded, in `dtype`.  decisions = (h1, h2, lv) fixes both LeakyReLU branches by the sign of
    the given activations and makes std = lv * softplus'(given lv): the linearisation whose autograd is the backward's reference"""
    p = lambda k: torch.from_numpy(sd['bodyprior_enc_' + k]).to(dtype)
    bn = lambda i, v: F.batch_norm(v, p(f'bn{i}.running_mean'), p(f'bn{i}.running_var'), p(f'bn{i}.weight'), p(f'bn{i}.bias'), False, 0.0, BN_EPS)
    slope = lambda h: torch.where(h > 0, torch.ones((), dtype=dtype), torch.full((), 0.2, dtype=dtype))
    a1 = F.linear(bn(1, x.to(dtype)), p('fc1.weight'), p('fc1.bias'))
    h1 = F.leaky_relu(a1, 0.2) if decisions is None else a1 * slope(decisions[0])
    a2 = F.linear(bn(2, h1), p('fc2.weight'), p('fc2.bias'))
    h2 = F.leaky_relu(a2, 0.2) if decisions is None else a2 * slope(decisions[1])
    mean, lv = F.linear(h2, p('mu.weight'), p('mu.bias')), F.linear(h2, p('logvar.weight'), p('logvar.bias'))
    if decisions is None:
        std = F.softplus(lv)
    else:
        l = decisions[2].to(dtype)
        std = lv * torch.where(l > 20, torch.ones((), dtype=dtype), torch.sigmoid(l))
    return dict(mean=mean, std=std, h1=h1, h2=h2, lv=lv)


def fold_terms(sd, x, ref):
    """the folded weights' rounding carried to every output (module docstring), each divided by max |ref| like err_of"""
    f = {k: torch.from_numpy(v).double() for k, v in fold_vposer_enc(sd).items()}
    xa = F.pad(x.double().abs(), (0, 1))
    E1 = U * (xa @ f['w1'].abs().t() + f['b1'].abs())
    E2 = U * (ref['h1'].abs() @ f['w2'].abs().t() + f['b2'].abs()) + E1 @ f['w2'].abs().t()
    Eh = E2 @ f['wh'].abs().t()
    E = dict(h1=E1, h2=E2, mean=Eh[:, :32], lv=Eh[:, 32:], std=Eh[:, 32:])
    return {k: float(E[k].max() / ref[k].abs().max()) for k in E}


def fold_terms_bwd(sd, dec, d_mean, d_std, ref_dx):
    f = {k: torch.from_numpy(v).double() for k, v in fold_vposer_enc(sd).items()}
    slope = lambda h: torch.where(h > 0, 1.0, 0.2).double()
    l = dec[2].double()
    dh = torch.cat([d_mean.double(), d_std.double() * torch.where(l > 20, torch.ones((), dtype=torch.float64), torch.sigmoid(l))], 1)
    d2 = (dh @ f['wh']) * slope(dec[1])
    d1 = (d2 @ f['w2']) * slope(dec[0])
    F1 = U * (d2.abs() @ f['w2'].abs())
    Ex = (U * (d1.abs() @ f['w1'].abs()) + F1 @ f['w1'].abs())[:, :63]
    return float(Ex.max() / ref_dx.abs().max())


@functools.lru_cache(maxsize=None)
def fwd_case(B, variant):
    """(state, x, float64 restatement, float32 restatement, fold terms): computed once, shared, never modified"""
    sd = variant_state(variant)
    x = poses(B, 100 + B)
    with torch.no_grad():
        r64, r32 = restate(sd, x, torch.float64), restate(sd, x, torch.float32)
    return sd, x, r64, r32, fold_terms(sd, x, r64)


_STRUCTS = {}


def weight_struct(sd, dev):
    key = (id(sd), str(dev))
    if key not in _STRUCTS:
        _STRUCTS[key] = vposer_enc_weight_struct(sd, dev) + (sd,)
    return _STRUCTS[key][0]


# ---------------------------------------------------------------------------------------------------------------------------
# buffers

def strided_rows(B, cols, stride, offset, values, dev):
    """guarded buffer of B rows `stride` apart, the first `offset` floats in, with `values` [B][cols] (or NaN) in them and NaN in every
    other element; nothing follows the last row's `cols` floats but the guard -> (whole, n, view that starts at row 0)"""
    n = offset + (B - 1) * stride + cols
    t = torch.full((n,), NAN)
    if values is not None:
        t[offset:].as_strided((B, cols), (stride, 1)).copy_(values)
    whole, view = guarded(n, dev)
    view.copy_(t.to(dev))
    return whole, n, view[offset:]


def rows_result(whole, n, B, cols, stride, offset, what):
    """guards intact, every element outside the B x cols rows still NaN, the rows finite -> [B][cols]"""
    v = guards_intact(whole, n, what)
    rows = v[offset:].as_strided((B, cols), (stride, 1)).clone()
    rest = v.clone()
    rest[offset:].as_strided((B, cols), (stride, 1)).fill_(NAN)
    assert torch.isnan(rest).all(), f'{what}: wrote outside its {cols} columns'
    assert torch.isfinite(rows).all(), f'{what}: rows not written (or not finite)'
    return rows


def run_fwd(lib, dev, sd, x, B, pin_stride=63, out_stride=32, pin_off=0, save=True, B_arg=None, null=(), strides=None):
    """one lemo_vposer_encode_fwd -> (rc, dict of (whole, n)); `null`: arguments passed as NULL; B_arg / strides: what the call is TOLD"""
    st = weight_struct(sd, dev)
    xw, xn, xv = strided_rows(B, 63, pin_stride, pin_off, x, dev)
    out = {}
    for k in ('mean', 'std'):
        out[k] = strided_rows(B, 32, out_stride, 0, None, dev)
    for k, c in (('h1', 512), ('h2', 512), ('lv', 32)):
        out[k] = strided_rows(B, c, c, 0, None, dev)
    arg = lambda k: None if (k in null or (not save and k in ('h1', 'h2', 'lv'))) else ptr(out[k][2])
    ps, os_ = strides or (pin_stride, out_stride)
    rc = lib.vposer_encode_fwd(C.byref(st), None if 'pin' in null else ptr(xv), ps, B if B_arg is None else B_arg, arg('mean'), arg('std'), os_,
                               arg('h1'), arg('h2'), arg('lv'), lib.stream(dev))
    _sync(lib)
    return rc, out


def fwd_results(out, B, out_stride, what, save=True):
    res = {k: rows_result(out[k][0], out[k][1], B, 32, out_stride, 0, f'{what} {k}') for k in ('mean', 'std')}
    for k, c in (('h1', 512), ('h2', 512), ('lv', 32)):
        if save:
            res[k] = rows_result(out[k][0], out[k][1], B, c, c, 0, f'{what} {k}')
        else:
            assert torch.isnan(out[k][0].cpu()).all(), f'{what}: wrote {k} although none was asked for'
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward

def check_fwd(lib, dev, B, variant):
    what = f'vposer_encode_fwd B {B} {variant}'
    sd, x, r64, r32, terms = fwd_case(B, variant)
    if variant in ('softplus', 'strided'):
        assert float(r64['lv'].max()) > 20 and float(r64['lv'].min()) < -20, 'the scaled logvar head does not reach both softplus branches'
    ps, os_, off = (165, 56, 3) if variant == 'strided' else (63, 32, 0)
    rc, out = run_fwd(lib, dev, sd, x, B, ps, os_, off)
    assert rc == 0, f'{what}: refused ({rc})'
    LAUNCHED.add('fwd')
    res = fwd_results(out, B, os_, what)
    for k in ('h1', 'h2', 'lv', 'mean', 'std'):
        gate_plus(f'vposer_enc fwd {k}', res[k], r32[k], r64[k], f'{what} {k}', terms[k])
    if variant == 'nosave':
        rc, out2 = run_fwd(lib, dev, sd, x, B, ps, os_, off, save=False)
        assert rc == 0, rc
        res2 = fwd_results(out2, B, os_, what + ' without h1 / h2 / lv', save=False)
        same_bits(res2['mean'], res['mean'], f'{what}: mean changes when h1 / h2 / lv are not saved')
        same_bits(res2['std'], res['std'], f'{what}: std changes when h1 / h2 / lv are not saved')


def check_fwd_refusals(lib, dev):
    B = 5
    sd, x = variant_state('plain'), poses(5, 7)
    for why, kw in (('B = 0', dict(B_arg=0)), ('B = -1', dict(B_arg=-1)), ('null pin', dict(null=('pin',))), ('null mean', dict(null=('mean',))),
                    ('null std', dict(null=('std',))), ('pin_stride 62', dict(strides=(62, 32))), ('out_stride 31', dict(strides=(63, 31)))):
        rc, out = run_fwd(lib, dev, sd, x, B, **kw)
        assert rc == ERR_ARG, f'vposer_encode_fwd {why}: {rc}'
        for k, (whole, n, _) in out.items():
            assert torch.isnan(whole.cpu()).all(), f'vposer_encode_fwd {why}: a refused call wrote {k}'
    assert lib.vposer_encode_fwd(None, None, 63, B, None, None, 32, None, None, None, lib.stream(dev)) == ERR_ARG


def check_large(lib, dev):
    """B = 65 537: rows past a 65 535-limited grid dimension; the first 64, the last 64 and 256 seeded rows against float64"""
    B = LARGE_B
    sd = variant_state('plain')
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 63, generator=g) * SIGMA
    sel = torch.cat([torch.arange(64), torch.arange(B - 64, B), torch.randint(64, B - 64, (256,), generator=g)])
    with torch.no_grad():
        r64, r32 = restate(sd, x[sel], torch.float64), restate(sd, x[sel], torch.float32)
    terms = fold_terms(sd, x[sel], r64)
    rc, out = run_fwd(lib, dev, sd, x, B)
    assert rc == 0, rc
    LAUNCHED.add('fwd')
    for k, c in (('mean', 32), ('std', 32), ('h1', 512), ('h2', 512), ('lv', 32)):
        v = guards_intact(out[k][0], out[k][1], f'large B {k}').view(B, c)
        assert torch.isfinite(v).all(), f'large B: rows of {k} not written'
        gate_plus(f'vposer_enc fwd {k}', v[sel], r32[k], r64[k], f'vposer_encode_fwd B {B} {k}', terms[k])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. backward

@functools.lru_cache(maxsize=None)
def bwd_case(B, which, variant):
    sd, x, r64, _, _ = fwd_case(B, variant)
    dec = tuple(r64[k].float() for k in ('h1', 'h2', 'lv'))                # the float64 forward rounded to float32
    assert (dec[0] != 0).all() and (dec[1] != 0).all(), 'a supplied activation is exactly 0: change the seed'
    assert torch.equal(dec[0] > 0, r64['h1'] > 0) and torch.equal(dec[1] > 0, r64['h2'] > 0)
    g = torch.Generator().manual_seed(200 + B)
    d_mean = torch.randn(B, 32, generator=g) if which in ('mean', 'both') else None
    d_std = torch.randn(B, 32, generator=g) if which in ('std', 'both') else None
    zero = torch.zeros(B, 32)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xl = x.to(dtype).requires_grad_(True)
        r = restate(sd, xl, dtype, decisions=dec)
        L = (r['mean'] * (zero if d_mean is None else d_mean).to(dtype)).sum() + (r['std'] * (zero if d_std is None else d_std).to(dtype)).sum()
        ref[dtype] = torch.autograd.grad(L, xl)[0]
    term = fold_terms_bwd(sd, dec, zero if d_mean is None else d_mean, zero if d_std is None else d_std, ref[torch.float64])
    return sd, dec, d_mean, d_std, ref[torch.float64], ref[torch.float32], term


def run_bwd(lib, dev, sd, dec, d_mean, d_std, B, pin_stride=63, out_stride=32, pin_off=0, B_arg=None, null=(), strides=None):
    st = weight_struct(sd, dev)
    d = lambda t: t.contiguous().to(dev)
    keep = [d(t) for t in dec]
    gm = None if d_mean is None else strided_rows(B, 32, out_stride, 0, d_mean, dev)
    gs = None if d_std is None else strided_rows(B, 32, out_stride, 0, d_std, dev)
    xw, xn, xv = strided_rows(B, 63, pin_stride, pin_off, None, dev)
    ps, os_ = strides or (pin_stride, out_stride)
    a = lambda i, k: None if k in null else ptr(keep[i])
    rc = lib.vposer_encode_bwd(C.byref(st), a(0, 'h1'), a(1, 'h2'), a(2, 'lv'), None if gm is None else ptr(gm[2]), None if gs is None else ptr(gs[2]),
                               os_, B if B_arg is None else B_arg, None if 'dpin' in null else ptr(xv), ps, lib.stream(dev))
    _sync(lib)
    return rc, (xw, xn)


def check_bwd(lib, dev, B, which, variant):
    what = f'vposer_encode_bwd B {B} d_{which} {variant}'
    sd, dec, d_mean, d_std, r64, r32, term = bwd_case(B, which, variant)
    ps, os_, off = (165, 56, 3) if variant == 'strided' else (63, 32, 0)
    rc, (xw, xn) = run_bwd(lib, dev, sd, dec, d_mean, d_std, B, ps, os_, off)
    assert rc == 0, f'{what}: refused ({rc})'
    LAUNCHED.add('bwd')
    dx = rows_result(xw, xn, B, 63, ps, off, what + ' dpin')
    gate_plus('vposer_enc bwd dpin', dx, r32, r64, what, term)
    if which != 'both':                                                    # NULL == a zero tensor, bit for bit
        zero = torch.zeros(B, 32)
        rc, (zw, zn) = run_bwd(lib, dev, sd, dec, zero if d_mean is None else d_mean, zero if d_std is None else d_std, B, ps, os_, off)
        assert rc == 0, rc
        same_bits(rows_result(zw, zn, B, 63, ps, off, what + ' zeros'), dx, f'{what}: a NULL gradient differs from a zero tensor')


def check_bwd_refusals(lib, dev):
    B = 5
    sd, dec, d_mean, d_std, *_ = bwd_case(17, 'both', 'plain')
    dec, d_mean, d_std = tuple(t[:B] for t in dec), d_mean[:B], d_std[:B]
    for why, kw in (('B = 0', dict(B_arg=0)), ('B = -1', dict(B_arg=-1)), ('null h1', dict(null=('h1',))), ('null h2', dict(null=('h2',))),
                    ('null lv', dict(null=('lv',))), ('pin_stride 62', dict(strides=(62, 32))), ('out_stride 31', dict(strides=(63, 31)))):
        rc, (xw, xn) = run_bwd(lib, dev, sd, dec, d_mean, d_std, B, **kw)
        assert rc == ERR_ARG, f'vposer_encode_bwd {why}: {rc}'
        assert torch.isnan(xw.cpu()).all(), f'vposer_encode_bwd {why}: a refused call wrote dpin'
    rc, _ = run_bwd(lib, dev, sd, dec, d_mean, d_std, B, null=('dpin',))
    assert rc == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the Python surface

def make_vp(lib, dev, seed=2):
    vp = VPoser(_lib=lib if lib.is_emu else None).eval()
    vp.load_state_dict({**vp.state_dict(), **{k: torch.from_numpy(v) for k, v in {**make_vposer_weights(seed), **enc_state(seed)}.items()}})
    return vp.to(dev)


def c_forward(lib, dev, sd, x):
    B = x.shape[0]
    rc, out = run_fwd(lib, dev, sd, x, B)
    assert rc == 0, rc
    return fwd_results(out, B, 32, 'C entry')


def check_encode_shapes_and_autograd(lib, dev):
    N = 19
    sd, x = enc_state(2), poses(19, 11)
    vp = make_vp(lib, dev)
    want = c_forward(lib, dev, sd, x)
    for shape in ((N, 1, 21, 3), (N, 21, 3), (N, 63)):
        q = vp.encode(x.view(shape).to(dev))
        assert isinstance(q, torch.distributions.normal.Normal) and q.mean.shape == (N, 32) and q.scale.shape == (N, 32)
        same_bits(q.mean.detach().cpu(), want['mean'], f'encode {shape}: mean differs from the C entry')
        same_bits(q.scale.detach().cpu(), want['std'], f'encode {shape}: std differs from the C entry')
    LAUNCHED.add('fwd')
    g = torch.Generator().manual_seed(3)
    gm, gs = torch.randn(N, 32, generator=g), torch.randn(N, 32, generator=g)
    dec = tuple(want[k] for k in ('h1', 'h2', 'lv'))
    for use_m, use_s in ((True, True), (True, False), (False, True)):
        Pin = x.view(N, 1, 21, 3).to(dev).requires_grad_(True)
        q = vp.encode(Pin)
        L = (q.mean * gm.to(dev)).sum() if use_m else 0
        L = L + ((q.scale * gs.to(dev)).sum() if use_s else 0)
        L.backward()
        rc, (xw, xn) = run_bwd(lib, dev, sd, dec, gm if use_m else None, gs if use_s else None, N)
        assert rc == 0, rc
        same_bits(Pin.grad.cpu().view(N, 63), rows_result(xw, xn, N, 63, 63, 0, 'C bwd'), f'autograd through encode (mean {use_m}, std {use_s}) differs from the C entry')
    LAUNCHED.add('bwd')
    Pin = x.to(dev).requires_grad_(True)
    vp.encode(Pin).mean.sum().backward()
    assert Pin.grad is not None and float(Pin.grad.abs().max()) > 0
    import pytest
    with pytest.raises(RuntimeError):
        vp.train().encode(x.to(dev))
    with pytest.raises(RuntimeError):
        vp(x.to(dev))
    vp.eval()


def check_repack(lib, dev):
    """another state_dict, and then a changed running_var alone, must reach the kernel"""
    x = poses(9, 12)
    vp = make_vp(lib, dev, seed=2)
    m2 = vp.encode(x.to(dev)).mean.detach().cpu()
    sd3 = enc_state(3)
    vp.load_state_dict({**vp.state_dict(), **{k: torch.from_numpy(v) for k, v in sd3.items()}})
    q = vp.encode(x.to(dev))
    assert not torch.equal(q.mean.detach().cpu(), m2), 'load_state_dict did not repack the encoder'
    for sd, scale in ((sd3, 1.0), (enc_state(3, 1.0, 1.5), 1.5)):
        if scale != 1.0:
            with torch.no_grad():
                vp.bodyprior_enc_bn1.running_var.mul_(scale)
            q = vp.encode(x.to(dev))
        with torch.no_grad():
            r64, r32 = restate(sd, x, torch.float64), restate(sd, x, torch.float32)
        terms = fold_terms(sd, x, r64)
        gate_plus('vposer_enc fwd mean', q.mean.detach().cpu(), r32['mean'], r64['mean'], f'encode after repack (running_var x {scale}) mean', terms['mean'])
        gate_plus('vposer_enc fwd std', q.scale.detach().cpu(), r32['std'], r64['std'], f'encode after repack (running_var x {scale}) std', terms['std'])


def check_forward_and_samples(lib, dev):
    N = 7
    x = poses(N, 13).view(N, 1, 21, 3).to(dev)
    vp = make_vp(lib, dev)
    e = torch.randn(N, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        for ot, key, shape in (('aa', 'pose_aa', (N, 1, 21, 3)), ('matrot', 'pose_matrot', (N, 1, 21, 9))):
            res = vp(x, output_type=ot, eps=e)
            assert sorted(res) == sorted(['mean', 'std', key]) and res[key].shape == shape
            same_bits(res[key].cpu(), vp.decode(res['mean'] + res['std'] * e, ot).cpu(), f'forward(eps) {ot} is not decode(mean + std * eps)')
        torch.manual_seed(8)
        res = vp(x, output_type='aa')                                      # the reference's own path: q_z.rsample()
        torch.manual_seed(8)
        z = vp.encode(x).rsample()
        same_bits(res['pose_aa'].cpu(), vp.decode(z, 'aa').cpu(), 'forward() is not decode(q_z.rsample())')
        np.random.seed(3)
        Z = torch.tensor(np.random.normal(0., 1., size=(5, 32)), dtype=torch.float32).to(dev)
        got = vp.train().sample_poses(5, seed=3)                           # sample_poses puts the module in eval(), like the reference
        assert not vp.training and got.shape == (5, 1, 21, 3)
        same_bits(got.cpu(), vp.decode(Z, 'aa').cpu(), 'sample_poses(5, seed=3) is not decode of numpy\'s draws')
        assert vp.sample_poses(2, output_type='matrot', seed=1).shape == (2, 1, 21, 9)


def check_rotation_helpers(lib, dev):
    N = 6
    aa = (torch.randn(N, 1, 21, 3, generator=torch.Generator().manual_seed(6)) * SIGMA).to(dev)
    R = VPoser.aa2matrot(aa)
    assert R.shape == (N, 1, 21, 9)
    back = VPoser.matrot2aa(R, _lib=lib if lib.is_emu else None)
    assert back.shape == (N, 1, 21, 3)
    R2 = VPoser.aa2matrot(back)
    assert float((R2 - R).abs().max()) <= 2.0 ** -20, float((R2 - R).abs().max())
    I = torch.eye(3, device=dev).view(1, 1, 1, 9).expand(N, 1, 21, 9)
    assert float((R - I).abs().max()) > 0.1                                # the rotations are not all near the identity


def check_embed(lib, dev):
    B = 11
    vp = make_vp(lib, dev)
    bp = poses(B, 14).to(dev)
    emb, err = embed_body_pose(vp, bp)
    assert emb.shape == (B, 32) and err.shape == (B,)
    with torch.no_grad():
        mean = vp.encode(bp).mean
        want = (vp.decode(mean, 'aa').view(B, 63) - bp).abs().amax(1)
    same_bits(emb.detach().cpu(), mean.cpu(), 'embed_body_pose: pose_embedding is not the encoder mean')
    same_bits(err.cpu(), want.cpu(), 'embed_body_pose: reproj_err is not max |decode(mean) - body_pose| per frame')
    same_bits(embed_body_pose(vp, bp.view(B, 21, 3))[0].detach().cpu(), mean.cpu(), 'embed_body_pose on [B, 21, 3]')


def check_with_pose_embedding(lib):
    """fills an absent key, hands a dict with the key back untouched, and the filled dict constructs a ProxTemporalFitter on the
    synthetic window of the prox tests (construction only)"""
    import __graft_entry__ as ge
    from lemo_amd.prox_windows import with_pose_embedding
    prob = ge.prox_small_problem(stage='S2')
    B = prob['B']
    vp = make_vp(lib, torch.device('cpu') if lib.is_emu else torch.device('cuda', 0))
    dev = vp.bodyprior_enc_fc1.weight.device
    params = dict(prob['params'])
    assert with_pose_embedding(params, vp) is params
    with torch.no_grad():
        bp = vp.decode(torch.from_numpy(params.pop('pose_embedding')).to(dev), 'aa').view(B, 63).cpu().numpy()
    params['body_pose'] = bp
    filled = with_pose_embedding(params, vp)
    assert 'pose_embedding' not in params and filled is not params and filled['pose_embedding'].shape == (B, 32)
    assert all(filled[k] is params[k] for k in params)
    with torch.no_grad():
        same_bits(torch.from_numpy(filled['pose_embedding']), vp.encode(torch.from_numpy(bp).to(dev)).mean.cpu(), 'with_pose_embedding: not the encoder mean')
    prob = dict(prob, params={k: v for k, v in filled.items() if k != 'body_pose'})
    fit, _ = ge.prox_fitter_for(prob, dev, lib=lib if lib.is_emu else None)
    assert fit.pose_embedding.shape == (B, 32)
    same_bits(fit.pose_embedding.detach().cpu(), torch.from_numpy(filled['pose_embedding']), 'the fitter does not start from the filled embedding')


# ---------------------------------------------------------------------------------------------------------------------------
# 4. against the reference's own run (tests/golden/make_vposer_encode.py)

def check_reference_run(lib, dev):
    from conftest import GOLDEN
    from oracle import lemo_oracle as O
    g = np.load(os.path.join(GOLDEN, 'vposer_encode.npz'))
    sd, dw = enc_state(2), make_vposer_weights(2)
    x = torch.from_numpy(g['Pin'])
    B = x.shape[0]
    with torch.no_grad():
        r64, r32 = restate(sd, x.view(B, 63), torch.float64), restate(sd, x.view(B, 63), torch.float32)
    # the restatement restates the reference: the recorded arrays lie within the gate of float64, the float32 restatement the yardstick
    gate('vposer_enc reference mean', torch.from_numpy(g['mean']), r32['mean'], r64['mean'], 'recorded reference mean')
    gate('vposer_enc reference std', torch.from_numpy(g['std']), r32['std'], r64['std'], 'recorded reference std')
    eps = torch.from_numpy(g['eps'])
    with torch.no_grad():
        aa64 = O.vposer_decode({k: torch.from_numpy(v).double() for k, v in dw.items()}, r64['mean'] + r64['std'] * eps, 'aa')
        aa32 = O.vposer_decode({k: torch.from_numpy(v) for k, v in dw.items()}, r32['mean'] + r32['std'] * eps.float(), 'aa')
    # ... and the recorded forward() is that float64 chain (the reference drew z = mean + std * eps)
    assert float((torch.from_numpy(g['pose_aa']).double() - aa64).abs().max() / aa64.abs().max()) < 1e-4
    vp = make_vp(lib, dev)
    terms = fold_terms(sd, x.view(B, 63), r64)
    with torch.no_grad():
        q = vp.encode(x.to(dev))
        res = vp(x.to(dev), output_type='aa', eps=eps.float().to(dev))
    gate_plus('vposer_enc fwd mean', q.mean.cpu(), r32['mean'], r64['mean'], 'encode on the reference fixture: mean', terms['mean'])
    gate_plus('vposer_enc fwd std', q.scale.cpu(), r32['std'], r64['std'], 'encode on the reference fixture: std', terms['std'])
    # pose_aa: the gate (yardstick: the float32 restatement of the whole chain) plus the shipped decoder's own 1e-4
    gate_plus('vposer_enc forward pose_aa', res['pose_aa'].cpu(), aa32, aa64, 'forward(eps) on the reference fixture: pose_aa', 1e-4)


def report_ratios():
    """the worst kernel / bound ratios of the cases above, and: forward and backward were both launched"""
    for k in sorted(RATIOS):
        if k.startswith('vposer_enc'):
            r, e, n = RATIOS[k]
            print(f'vposer_enc ratio {k}: worst 4 x kernel error / bound {r:.2f}, worst kernel error {e:.3e} ({n} comparisons)')
    print(f'launched: {sorted(LAUNCHED)}')
    assert LAUNCHED == {'fwd', 'bwd'}, f'not launched: {sorted({"fwd", "bwd"} - LAUNCHED)}'
