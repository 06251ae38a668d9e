"""Direct tests of the body-model kernels through their own C entry points, against float64 on the CPU (tests/test_lbs_emu.py on
the host-emulated build, tests/test_lbs_gpu.py on the MI355X; both run the cases below):

  lemo_lbs_verts_fwd / _xs            blend GEMM + skinning, four launchable forms              csrc/lbs_kernels.hip
  lemo_lbs_verts_fwd_active           the same over a small vertex set (gemm_nt16_kg8 + skin)   csrc/lbs_kernels.hip, gemm_kernels.hip
  lemo_lbs_verts_bwd                  its adjoint, five routes                                  csrc/lbs_kernels.hip
  lemo_smplx_pose_fwd / _bwd          hand PCA, Rodrigues, joint regression, kinematic chain    csrc/pose_kernels.hip
  lemo_joints_assemble                posed joints | vertex picks | landmarks                   csrc/lbs_kernels.hip
  lemo_rot6d_to_aa_fwd / _bwd         6-D -> axis-angle head                                    csrc/rot.hpp
  lemo_vposer_decode_fwd / _bwd       its rotation part only (the MLP GEMM is in blocks_common) csrc/pose_kernels.hip, rot.hpp

Operands are built here, not by the engines: a small random SkinConst (V, nj, KW chosen per case; ELL rows that sum to 1, some
padded with weight 0), random features Xg and random rigid transforms A -- which is what lets nj leave the 55 of every model in the
suite.  The scales are chosen so that the blend (sigma 0.25) is as large as the template (sigma 0.25): an error of the blend GEMM
then shows in v_posed at full size instead of hiding under the template's rounding.  Layouts come from the repository's helpers
(BodyModelData.vertex_set, split_f16_pairs, bf16_split3) and from alloc_pose_ws's statement of Xg / XgS.

Buffers: every input a form does not read holds NaN (Xg when XgS is given; Dg when DgH is given; rows of v_posed outside vp_row;
the split-K and chunk workspaces); the Xg pad rows (features >= 506) and pad frames (>= B) are zero; every output sits between
GUARD sentinels and is pre-filled with NaN; a refused call must leave them so.

Tolerances
----------
err(v) = max |v - ref| / max |ref| against float64 formed from the same float32 inputs.  The yardstick is a float32 CPU restatement
(torch float32 matmul + float32 skinning, or float32 autograd of it): blocks_common.gate, GATE = 4, floor 2^-23 where the
restatement is exact.  Never another kernel form.
* fp32 MFMA and the three-piece bf16 split multiply exact operands: nothing extra.
* The fp16 form multiplies D' = D (1 + d), X' = X (1 + e) with |d|, |e| <= 2^-22 (two fp16 pieces hold 22 significand bits; the
  test checks on the host that its Dg and Xg do meet that), so a product is off by <= (2^-22 + 2^-22) |D X| = 2^-21 |D X| to first
  order.  v_posed_c = sum_k D_kc X_k is then off by <= 2^-21 sum_k |D_kc| |X_k| and, through verts_r = sum_c T_rc v_posed_c + ..,
  verts_r by <= 2^-21 sum_c |T_rc| sum_k |D_kc| |X_k|.  The largest of these over the outputs, divided by max |ref| like err,
  is added to the gate's bound for this form only.  (The dropped lo x lo product is < 2^-22 |D X| in the worst case and 2^-24
  sized in practice; it is left to the 4 x restatement part.)
* Bit checks: bf16 with XgS == bf16 converting in the kernel; a subset run == the same rows of the all-vertex run; the
  order-fixed backward routes twice == equal bits; joints_assemble's `Jtr + transl` (one IEEE addition) and picks == equal bits.
* Landmarks: a three-term float32 sum of products, |got - ref| <= 3 * 2^-24 * sum |terms|.
* dvp columns 3 n .. NCs - 1 are exactly 0 after every backward route."""
import ctypes as C
import os
import types

import numpy as np
import torch

from blocks_common import ERR_ARG, ERR_SHAPE, FLOOR, GATE, NAN, RATIOS, U, _sync, err_of, gate, guarded, guards_intact, same_bits
from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.body_model import K_PAD, BodyModelData, split_f16_pairs
from lemo_amd.priors import bf16_split3

KFEAT = 506                       # 20 shape / expression + 486 pose features; 506 .. 511 are the pad rows of Xg (zero)
FORMS = ('fp32', 'bf16', 'bf16_xs', 'f16')
F16_EPS = 2.0 ** -21


def _roundup(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def make_skin(V, nj, KW, seed, full=False, empty_joint=None, full_joint=None):
    """a random SkinConst in numpy: D [512][3 V] (rows >= KFEAT zero), Dg [64][NC][8], v_template, ELL weights [V][KW] whose rows
    sum to 1; a row has 1 .. KW entries (`full`: exactly KW), the rest padded with (joint 0, weight 0) as BodyModelData does"""
    rng = np.random.default_rng(seed)
    D = np.zeros((K_PAD, 3 * V), np.float32)
    D[:KFEAT] = rng.standard_normal((KFEAT, 3 * V)) * 0.037             # x features of sigma 0.3: blend of sigma 0.25
    NC = _roundup(3 * V, 8)
    Dg = np.zeros((K_PAD // 8, NC, 8), np.float32)
    Dg[:, :3 * V, :] = D.reshape(K_PAD // 8, 8, 3 * V).transpose(0, 2, 1)
    pool = np.array([j for j in range(nj) if j not in (empty_joint, full_joint)])
    w_idx, w_val = np.zeros((V, KW), np.int32), np.zeros((V, KW), np.float32)
    for v in range(V):
        m = KW if full else 1 + int(rng.integers(KW))
        j = pool[rng.permutation(len(pool))[:m]]
        if full_joint is not None:
            j[0] = full_joint
        w = (rng.random(m) + 0.05).astype(np.float32)
        w_idx[v, :m], w_val[v, :m] = j, w / w.sum()
    assert KW == 1 or full or (w_val == 0).any(), 'no padded ELL row'
    return types.SimpleNamespace(V=V, nj=nj, KW=KW, NC=NC, D=D, Dg=Dg, v_template=(rng.standard_normal((V, 3)) * 0.25).astype(np.float32),
                                 w_idx=w_idx, w_val=w_val)


def skin_const(sk, dev, form='fp32'):
    """(lemo_skin_const, tensors that keep it alive).  'f16': DgH from split_f16_pairs and NaN in the fp32 copy, which that form
    must not read"""
    t = {k: torch.from_numpy(getattr(sk, k)).to(dev) for k in ('v_template', 'w_idx', 'w_val')}
    inv = 0.0
    if form == 'f16':
        h, inv = split_f16_pairs(sk.Dg)
        t['DgH'] = torch.from_numpy(h).to(dev)
        t['Dg'] = torch.full(sk.Dg.shape, NAN).to(dev)
    else:
        t['Dg'] = torch.from_numpy(sk.Dg).to(dev)
    st = _hip.SkinConst(sk.V, sk.NC, sk.KW, 1 if form == 'fp32' else 0, ptr(t['Dg']), ptr(t['v_template']), ptr(t['w_idx']), ptr(t['w_val']),
                        ptr(t.get('DgH')), inv)
    return st, t


def rigid_transforms(B, nj, g):
    """[B][nj][3][4] float32: a rotation (Rodrigues in float64) and a translation of sigma 0.5"""
    aa = torch.randn(B, nj, 3, generator=g, dtype=torch.float64)
    th = aa.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    k = aa / th
    Kx = torch.zeros(B, nj, 3, 3, dtype=torch.float64)
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    s, c = torch.sin(th)[..., None], torch.cos(th)[..., None]
    R = torch.eye(3, dtype=torch.float64) + s * Kx + (1 - c) * (Kx @ Kx)
    t = torch.randn(B, nj, 3, 1, generator=g, dtype=torch.float64) * 0.5
    return torch.cat([R, t], -1).float().contiguous()


def features(B, g):
    """X [B][512] float32, sigma 0.3, pad features zero"""
    X = torch.zeros(B, K_PAD)
    X[:, :KFEAT] = torch.randn(B, KFEAT, generator=g) * 0.3
    return X


def xg_layout(X, Bp):
    """Xg[k >> 3][frame][k & 7], frames B .. Bp - 1 zero (alloc_pose_ws)"""
    B = X.shape[0]
    Xg = torch.zeros(K_PAD // 8, Bp, 8)
    Xg[:, :B] = X.view(B, K_PAD // 8, 8).permute(1, 0, 2)
    return Xg


def xgs_layout(X, Bp, f16):
    """XgS[k >> 4][piece][frame][(k >> 3) & 1][k & 7] as int16 bits: three exact bf16 pieces, or hi = f16(x), lo = f16(x - hi)"""
    B = X.shape[0]
    x = X.numpy()
    if f16:
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        bits = np.stack([hi, lo], 0).view(np.int16)
    else:
        bits = (np.stack(bf16_split3(x), 0).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    P = bits.shape[0]
    out = np.zeros((K_PAD // 16, P, Bp, 2, 8), np.int16)
    out[:, :, :B] = bits.reshape(P, B, K_PAD // 16, 2, 8).transpose(2, 0, 1, 3, 4)
    return torch.from_numpy(out)


def dense_weights(sk, dtype):
    Wd = torch.zeros(sk.V, sk.nj, dtype=dtype)
    Wd.scatter_add_(1, torch.from_numpy(sk.w_idx).long(), torch.from_numpy(sk.w_val).to(dtype))
    return Wd


def lbs_reference(sk, X, A, transl, ids, dtype, vp=None):
    """(verts, v_posed, T) [B][n][3] in `dtype` from the float32 operands: v_posed = v_template + X . D, verts = (sum_j W A_j) [v_posed, 1]
    (+ transl).  `vp`: skin these v_posed rows instead of blending"""
    idl = torch.as_tensor(ids).long()
    B = A.shape[0]
    if vp is None:
        cols = (idl[:, None] * 3 + torch.arange(3)[None]).reshape(-1)
        vp = (X.to(dtype) @ torch.from_numpy(sk.D).to(dtype)[:, cols]).reshape(B, -1, 3) + torch.from_numpy(sk.v_template).to(dtype)[idl]
    T = torch.einsum('vj,bjrc->bvrc', dense_weights(sk, dtype)[idl], A.to(dtype))
    verts = torch.einsum('bvrc,bvc->bvr', T[..., :3], vp) + T[..., 3]
    if transl is not None:
        verts = verts + transl.to(dtype)[:, None]
    return verts, vp, T


def gate_plus(family, got, f32, ref, what, extra):
    """blocks_common.gate with `extra` (already normalised like err_of) added to the bound: the fp16 form's operand term"""
    if not extra:
        return gate(family, got, f32, ref, what)
    assert torch.isfinite(got).all(), what
    e_k, e_32 = err_of(got, ref), err_of(f32, ref)
    bound = (GATE * e_32 if e_32 > 0 else FLOOR) + extra
    ratio = GATE * e_k / bound
    r, e, n = RATIOS.get(family, (0.0, 0.0, 0))
    RATIOS[family] = (max(r, ratio), max(e, e_k), n + 1)
    print(f'{what}: kernel {e_k:.3e} restatement {e_32:.3e} operand term {extra:.3e} ratio {ratio:.2f}')
    assert e_k <= bound, f'{what}: {e_k:.3e} from float64, bound {bound:.3e} = {GATE:g} x {e_32:.3e} + {extra:.3e}'
    return e_k


FORMS_RUN, ROUTES_RUN = set(), set()                  # what check_fwd / check_bwd launched in this process


def report_lbs_ratios():
    """the ratios, and: all four forward forms and all five backward routes ran (the last test of either driver)"""
    from blocks_common import report_ratios
    report_ratios()
    print(f'forward forms run: {sorted(FORMS_RUN)}; backward routes run: {sorted(ROUTES_RUN)}')
    assert FORMS_RUN == set(FORMS), f'forward forms not run: {sorted(set(FORMS) - FORMS_RUN)}'
    want = {c[0] for c in BWD_CASES.values()}
    assert len(want) == 5 and ROUTES_RUN == want, f'backward routes not run: {sorted(want - ROUTES_RUN)}'


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lemo_lbs_verts_fwd / _xs: tiles of 42 vertices x 128 frames, skinning in 12-frame chunks, the fifth A staging load at nj >= 57

def _fwd_cases():
    """seven cases per form: every B, every vertex count and every nj / KW / null choice appears with every form; the pairing is
    rotated from form to form.  (V, n or None for all vertices)"""
    Bs = (1, 12, 13, 32, 33, 128, 129)
    verts = ((1, None), (42, None), (43, None), (127, None), (43, 1), (127, 41), (127, 85))
    njs, kws = (55, 57, 64), (1, 4, 11)
    out = []
    for f, form in enumerate(FORMS):
        for i, B in enumerate(Bs):
            V, n = verts[(i + 2 * f) % 7]
            out.append((form, V, n, njs[(i + f) % 3], kws[(i + 2 * f + i // 3) % 3], B, (i + f) % 2 == 0, (i + f) % 3 != 1))
    return out


FWD_CASES = _fwd_cases()


def subset_ids(V, n, g):
    """n ids out of V, unsorted, one of them repeated (n >= 2)"""
    ids = torch.randperm(V, generator=g)[:n].int()
    if n >= 2:
        ids[n - 1] = ids[0]
    return ids.contiguous()


def fwd_operands(form, V, n, nj, KW, B, seed):
    g = torch.Generator().manual_seed(seed)
    sk = make_skin(V, nj, KW, seed)
    X, A, tr = features(B, g), rigid_transforms(B, nj, g), torch.randn(B, 3, generator=g)
    ids = None if n is None else subset_ids(V, n, g)
    return sk, X, A, tr, ids


def run_fwd(lib, dev, form, sk, X, A, tr, ids, want_vp, what, nj=None):
    """one launch in `form` -> (rc, verts whole, v_posed whole, n)"""
    B = X.shape[0]
    Bp = _roundup(B, 32)
    n = sk.V if ids is None else len(ids)
    st, keep = skin_const(sk, dev, form)
    pre = form in ('bf16_xs', 'f16')
    Xg = (torch.full((K_PAD // 8, Bp, 8), NAN) if pre else xg_layout(X, Bp)).to(dev)      # a pre-split launch must not read Xg
    XgS = xgs_layout(X, Bp, form == 'f16').to(dev) if pre else None
    Ad, trd, idd = A.to(dev), None if tr is None else tr.to(dev), None if ids is None else ids.to(dev)
    vwhole, v = guarded(B * n * 3, dev)
    pwhole, vp = guarded(B * n * 3, dev)
    nj = sk.nj if nj is None else nj
    if pre:
        rc = lib.lbs_verts_fwd_xs(C.byref(st), ptr(Xg), ptr(XgS), Bp, ptr(Ad), nj, ptr(trd), ptr(idd), n, B, ptr(v), ptr(vp) if want_vp else None,
                                  lib.stream(dev))
    else:
        rc = lib.lbs_verts_fwd(C.byref(st), ptr(Xg), Bp, ptr(Ad), nj, ptr(trd), ptr(idd), n, B, ptr(v), ptr(vp) if want_vp else None, lib.stream(dev))
    _sync(lib)
    return rc, vwhole, pwhole, n


def f16_terms(sk, X, T, ids, ref_v, ref_p):
    """the fp16 form's operand terms for (verts, v_posed), see the module docstring; also checks that the pieces hold 2^-22"""
    h, inv = split_f16_pairs(sk.Dg)
    hp = h.view(np.float16).reshape(sk.Dg.shape[0], sk.Dg.shape[1], 2, 2, 4).astype(np.float64)
    back = (hp[:, :, :, 0, :] + hp[:, :, :, 1, :]).reshape(sk.Dg.shape) * inv
    assert np.abs(back - sk.Dg).max() <= np.abs(sk.Dg).max() * 2.0 ** -21, 'split_f16_pairs misses 2^-21 of the largest entry'
    idl = torch.arange(sk.V) if ids is None else ids.long()
    cols = (idl[:, None] * 3 + torch.arange(3)[None]).reshape(-1)
    S = (X.double().abs() @ torch.from_numpy(sk.D).double().abs()[:, cols]).reshape(X.shape[0], -1, 3)
    ev = F16_EPS * float(torch.einsum('bvrc,bvc->bvr', T[..., :3].abs(), S).max() / ref_v.abs().max())
    ep = F16_EPS * float(S.max() / ref_p.abs().max())
    return ev, ep


def check_fwd(lib, dev, form, V, n, nj, KW, B, with_transl, want_vp):
    what = f'lbs_verts_fwd {form} V {V} n {n} nj {nj} KW {KW} B {B} transl {with_transl} v_posed {want_vp}'
    sk, X, A, tr, ids = fwd_operands(form, V, n, nj, KW, B, seed=V * 1000 + nj * 10 + KW + B)
    if not with_transl:
        tr = None
    idr = torch.arange(V) if ids is None else ids
    ref_v, ref_p, T = lbs_reference(sk, X, A, tr, idr, torch.float64)
    f32_v, f32_p, _ = lbs_reference(sk, X, A, tr, idr, torch.float32)
    ev, ep = f16_terms(sk, X, T, ids, ref_v, ref_p) if form == 'f16' else (0.0, 0.0)
    rc, vwhole, pwhole, nn = run_fwd(lib, dev, form, sk, X, A, tr, ids, want_vp, what)
    assert rc == 0, f'{what}: refused ({rc})'
    v = guards_intact(vwhole, B * nn * 3, what + ' verts').view(B, nn, 3)
    p = guards_intact(pwhole, B * nn * 3, what + ' v_posed').view(B, nn, 3)
    FORMS_RUN.add(form)
    gate_plus(f'lbs_fwd {form} verts', v, f32_v, ref_v, what + ' verts', ev)
    if want_vp:
        gate_plus(f'lbs_fwd {form} v_posed', p, f32_p, ref_p, what + ' v_posed', ep)
    else:
        assert torch.isnan(p).all(), f'{what}: wrote v_posed although none was asked for'


BITS_CASES = ((127, 57, 4, 13), (43, 64, 11, 129))      # (V, nj, KW, B)


def check_fwd_bits(lib, dev, V, nj, KW, B):
    """bf16 with XgS == bf16 without; in every form a subset run == the same rows of the all-vertex run"""
    sk, X, A, tr, _ = fwd_operands('bits', V, None, nj, KW, B, seed=V + nj + KW + B)
    ids = subset_ids(V, min(V, 85) - 2, torch.Generator().manual_seed(V))
    alls = {}
    for form in FORMS:
        what = f'lbs_verts_fwd bits {form} V {V} nj {nj} KW {KW} B {B}'
        rc, vw, pw, _ = run_fwd(lib, dev, form, sk, X, A, tr, None, True, what)
        assert rc == 0, rc
        v, p = guards_intact(vw, B * V * 3, what).view(B, V, 3).clone(), guards_intact(pw, B * V * 3, what).view(B, V, 3).clone()
        assert torch.isfinite(v).all() and torch.isfinite(p).all(), what
        alls[form] = (v, p)
        rc, vw, pw, n = run_fwd(lib, dev, form, sk, X, A, tr, ids, True, what + ' subset')
        assert rc == 0, rc
        same_bits(guards_intact(vw, B * n * 3, what).view(B, n, 3), v[:, ids.long()], f'{what}: subset verts differ from the all-vertex rows')
        same_bits(guards_intact(pw, B * n * 3, what).view(B, n, 3), p[:, ids.long()], f'{what}: subset v_posed differ from the all-vertex rows')
    same_bits(alls['bf16'][0], alls['bf16_xs'][0], 'bf16: pre-split XgS changes verts')
    same_bits(alls['bf16'][1], alls['bf16_xs'][1], 'bf16: pre-split XgS changes v_posed')


def check_xgs_layouts():
    """the test's own XgS: three bf16 pieces resum to Xg exactly, two fp16 pieces to 2^-21 of the largest entry (host only)"""
    X = features(5, torch.Generator().manual_seed(2))
    Bp = 32
    xg = xg_layout(X, Bp).view(-1, 2, Bp, 8).permute(0, 2, 1, 3).double()                 # [K/16][Bp][2][8]
    b = ((xgs_layout(X, Bp, False).to(torch.int32) & 0xFFFF) << 16).view(torch.float32).double().sum(1)
    assert torch.equal(b, xg) and float(xg.abs().max()) > 0.5
    h = xgs_layout(X, Bp, True).view(torch.float16).double().sum(1)
    assert float((h - xg).abs().max()) <= float(xg.abs().max()) * 2.0 ** -21


def check_fwd_refusals(lib, dev):
    """nj = 65 and the shape refusals: LEMO_ERR_SHAPE, outputs untouched"""
    V, B = 43, 3
    g = torch.Generator().manual_seed(9)
    sk = make_skin(V, 64, 4, 9)
    X, tr = features(B, g), torch.randn(B, 3, generator=g)
    ids = subset_ids(V, 5, g)
    for form in FORMS:
        for nj, ids_, n_over, B_over, why in ((65, None, None, None, 'nj = 65'), (64, None, V - 1, None, 'n != V without ids'),
                                              (64, ids, 0, None, 'n = 0'), (64, None, None, 33, 'B > Bp')):
            A = rigid_transforms(max(B, B_over or 0), nj, g)
            st, keep = skin_const(sk, dev, form)
            Bp = 32
            pre = form in ('bf16_xs', 'f16')
            Xg, XgS = xg_layout(X, Bp).to(dev), xgs_layout(X, Bp, form == 'f16').to(dev) if pre else None
            Ad, trd, idd = A.to(dev), tr.to(dev), None if ids_ is None else ids_.to(dev)
            n = V if n_over is None else n_over
            Bc = B if B_over is None else B_over
            vwhole, v = guarded(40 * V * 3, dev)
            pwhole, p = guarded(40 * V * 3, dev)
            if pre:
                rc = lib.lbs_verts_fwd_xs(C.byref(st), ptr(Xg), ptr(XgS), Bp, ptr(Ad), nj, ptr(trd), ptr(idd), n, Bc, ptr(v), ptr(p), lib.stream(dev))
            else:
                rc = lib.lbs_verts_fwd(C.byref(st), ptr(Xg), Bp, ptr(Ad), nj, ptr(trd), ptr(idd), n, Bc, ptr(v), ptr(p), lib.stream(dev))
            _sync(lib)
            assert rc == ERR_SHAPE, f'{form} {why}: {rc}'
            assert torch.isnan(vwhole.cpu()).all() and torch.isnan(pwhole.cpu()).all(), f'{form} {why}: a refused launch wrote its outputs'


# ---------------------------------------------------------------------------------------------------------------------------
# vertex sets: BodyModelData.vertex_set on the random skin + hand-set scratch fields

def vertex_set(sk, ids, vp_row, dev, tables=None, frames=0, gemm_slabs=0, dkg=False, dkt=True):
    """(lemo_vertex_set_bwd, tensors, numpy dict).  `tables`: None = as vertex_set decides (n > 1024); scratch (`part`, `gemm_part`) is
    allocated here, guarded and full of NaN"""
    s = BodyModelData.vertex_set(sk, np.asarray(ids), None if vp_row is None else np.asarray(vp_row))
    if tables is False:
        for k in ('jcsr_chunk', 'jc_u', 'jc_w'):
            s.pop(k, None)
    tt = {k: torch.from_numpy(v).to(dev) for k, v in s.items() if isinstance(v, np.ndarray)}
    st = _hip.VertexSetBwd(s['n'], s['NCs'], ptr(tt['ids']), ptr(tt['vp_row']), ptr(tt['Dk']), ptr(tt['DkT']) if dkt and 'DkT' in tt else None,
                           ptr(tt['jcsr_start']), ptr(tt['jcsr_u']), ptr(tt['jcsr_w']), ptr(tt.get('jcsr_chunk')), ptr(tt.get('jc_u')), ptr(tt.get('jc_w')),
                           None, 0)
    if frames:
        nchunk = (s['n'] + 511) // 512
        tt['part_whole'], tt['part'] = guarded(frames * nchunk * (sk.nj * 12 + 4), dev)
        st.part, st.part_frames = ptr(tt['part']), frames
    if gemm_slabs:
        npart = gemm_slabs * 128 * K_PAD
        tt['gemm_part_whole'], tt['gemm_part'] = guarded(npart, dev)
        st.gemm_part, st.gemm_slabs = ptr(tt['gemm_part']), gemm_slabs
        if dkg:
            tt['DkG'] = tt['Dk'].view(K_PAD, s['NCs'] // 16, 16).permute(1, 0, 2).contiguous()
            st.DkG = ptr(tt['DkG'])
    return st, tt, s


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lemo_lbs_verts_fwd_active: gemm_nt16_kg8 over DkT [NCs][512], then a thread per (frame, vertex) that rounds KW up to 4

ACTIVE_CASES = ((1, 1, 3), (5, 17, 4), (253, 33, 5), (5, 33, 3), (253, 1, 4), (1, 17, 5))     # (n, B, KW): NCs = 16, 16, 768


def active_operands(n, B, KW, seed):
    g = torch.Generator().manual_seed(seed)
    V, nj = n + 30, 55
    sk = make_skin(V, nj, KW, seed)
    ids = torch.randperm(V, generator=g)[:n].int()
    return sk, features(B, g), rigid_transforms(B, nj, g), torch.randn(B, 3, generator=g), ids


def check_active(lib, dev, n, B, KW, with_transl=True, want_vp=True):
    what = f'lbs_verts_fwd_active n {n} B {B} KW {KW}'
    sk, X, A, tr, ids = active_operands(n, B, KW, seed=n * 100 + B * 7 + KW)
    if not with_transl:
        tr = None
    ref_v, ref_p, _ = lbs_reference(sk, X, A, tr, ids, torch.float64)
    f32_v, f32_p, _ = lbs_reference(sk, X, A, tr, ids, torch.float32)
    st, keep = skin_const(sk, dev)
    u, ut, s = vertex_set(sk, ids.numpy(), None, dev)
    assert s['NCs'] == _roundup(3 * n, 16) and u.DkT
    Bp = _roundup(B, 32)
    Xg, Ad, trd = xg_layout(X, Bp).to(dev), A.to(dev), None if tr is None else tr.to(dev)
    bwhole, blend = guarded(B * s['NCs'], dev)
    vwhole, v = guarded(B * n * 3, dev)
    pwhole, p = guarded(B * n * 3, dev)
    rc = lib.lbs_verts_fwd_active(C.byref(st), C.byref(u), ptr(Xg), Bp, ptr(Ad), sk.nj, ptr(trd), B, ptr(blend), ptr(v), ptr(p) if want_vp else None,
                                  lib.stream(dev))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    guards_intact(bwhole, B * s['NCs'], what + ' blend')                # its pad columns may hold anything
    gate('lbs_fwd_active verts', guards_intact(vwhole, B * n * 3, what + ' verts').view(B, n, 3), f32_v, ref_v, what + ' verts')
    pp = guards_intact(pwhole, B * n * 3, what + ' v_posed').view(B, n, 3)
    if want_vp:
        gate('lbs_fwd_active v_posed', pp, f32_p, ref_p, what + ' v_posed')
    else:
        assert torch.isnan(pp).all()


def check_active_refusals(lib, dev):
    n, B, KW = 5, 3, 4
    sk, X, A, tr, ids = active_operands(n, B, KW, seed=4)
    st, keep = skin_const(sk, dev)
    Xg, Ad, trd = xg_layout(X, 32).to(dev), rigid_transforms(40, sk.nj, torch.Generator().manual_seed(1)).to(dev), torch.randn(40, 3).to(dev)
    for why in ('no DkT', 'NCs % 16', 'B > Bp', 'NCs < 3 n'):
        u, ut, s = vertex_set(sk, ids.numpy(), None, dev, dkt=why != 'no DkT')
        Bc = B
        if why == 'NCs % 16':
            u.NCs = 24
        if why == 'NCs < 3 n':
            u.n = 6
        if why == 'B > Bp':
            Bc = 33
        bwhole, blend = guarded(40 * 32, dev)
        vwhole, v = guarded(40 * 6 * 3, dev)
        pwhole, p = guarded(40 * 6 * 3, dev)
        rc = lib.lbs_verts_fwd_active(C.byref(st), C.byref(u), ptr(Xg), 32, ptr(Ad), sk.nj, ptr(trd), Bc, ptr(blend), ptr(v), ptr(p), lib.stream(dev))
        _sync(lib)
        assert rc == ERR_SHAPE, f'{why}: {rc}'
        assert torch.isnan(bwhole.cpu()).all() and torch.isnan(vwhole.cpu()).all() and torch.isnan(pwhole.cpu()).all(), f'{why}: a refused launch wrote'


# ---------------------------------------------------------------------------------------------------------------------------
# 3. lemo_lbs_verts_bwd, every route

def bwd_route(n, KW, nj, B, u):
    """the host arithmetic of lbs_verts_bwd, restated: which kernels the operands select"""
    assert 'LEMO_LBS_TWO_REDUCES' not in os.environ
    if n <= 1024 and nj <= 64 and n * KW <= 4096:
        return 'staged'
    if nj <= 64 and u.jcsr_chunk and u.jc_u and u.jc_w and u.part and B <= u.part_frames:
        return 'chunk + gemm_reduce' if u.gemm_part and u.gemm_slabs > 0 and B <= 128 else 'chunk + reduce'
    return 'atomics' if nj <= 64 else 'frame'


# name -> (route, V, n, nj, KW, B, options)
BWD_CASES = {
    'staged n1': ('staged', 9, 1, 55, 4, 3, dict(permute=True, special=True)),
    'staged n253 no dtransl': ('staged', 300, 253, 55, 4, 3, dict(permute=True, special=True, dtransl=False)),
    'staged n1024': ('staged', 1040, 1024, 55, 4, 2, dict(permute=True, special=True)),
    'atomics n640 KW11': ('atomics', 650, 640, 55, 11, 3, dict()),
    'chunk ident KW4 B2 no dtransl': ('chunk + gemm_reduce', 1030, 1030, 55, 4, 2, dict(frames=2, gemm_slabs=8, dtransl=False, twice=True)),
    'chunk subset KW6 B128 DkG': ('chunk + gemm_reduce', 1040, 1030, 55, 6, 128, dict(frames=128, gemm_slabs=8, dkg=True, full=True, twice=True)),
    'chunk ident KW6 B2 no gemm_part': ('chunk + reduce', 1025, 1025, 55, 6, 2, dict(frames=2, full=True, twice=True)),
    'chunk subset KW4 B129': ('chunk + reduce', 1030, 1025, 55, 4, 129, dict(frames=129, gemm_slabs=8, twice=True)),
    'frame nj65': ('frame', 40, 30, 65, 4, 2, dict()),
}


def bwd_reference(sk, ids, A, vp_sel, tr, dverts, Dk3, dtype):
    """(dvp [B][3 n], dA [B][nj][12], dtransl [B][3], dX [B][512]) by autograd of lbs_reference in `dtype`"""
    B, n = dverts.shape[:2]
    Al, vl, tl = A.to(dtype).requires_grad_(True), vp_sel.to(dtype).requires_grad_(True), tr.to(dtype).requires_grad_(True)
    X0 = torch.zeros(B, K_PAD, dtype=dtype, requires_grad=True)
    vp = vl + (X0 @ Dk3.to(dtype)).view(B, n, 3)
    verts, _, _ = lbs_reference(sk, None, Al, tl, ids, dtype, vp=vp)
    dA, dvp, dtr, dX = torch.autograd.grad(verts, (Al, vl, tl, X0), dverts.to(dtype))
    return dvp.reshape(B, 3 * n), dA.reshape(B, sk.nj, 12), dtr, dX


def check_bwd(lib, dev, name):
    route, V, n, nj, KW, B, o = BWD_CASES[name]
    what = f'lbs_verts_bwd {name}'
    g = torch.Generator().manual_seed(V + n + nj + KW + B)
    special = o.get('special')
    sk = make_skin(V, nj, KW, V + n, full=o.get('full', False), empty_joint=7 if special else None, full_joint=3 if special else None)
    ident = n == V
    ids = np.arange(V) if ident else torch.randperm(V, generator=g)[:n].numpy()
    if o.get('permute'):                                   # compact v_posed in another order than the set: vp_row != ids, vp_rows = n
        vp_row, vp_rows = torch.randperm(n, generator=g).numpy(), n
    else:                                                  # v_posed of the whole model (+ 3 rows nobody reads)
        vp_row, vp_rows = ids, V if ident else V + 3
    st, keep = skin_const(sk, dev)
    u, ut, s = vertex_set(sk, ids, vp_row, dev, frames=o.get('frames', 0), gemm_slabs=o.get('gemm_slabs', 0), dkg=o.get('dkg', False))
    NCs = s['NCs']
    assert bwd_route(n, KW, nj, B, u) == route, f'{what}: the operands select {bwd_route(n, KW, nj, B, u)}, not {route}'
    if route.startswith('chunk'):
        tab = s['jcsr_chunk']
        nnz = tab[:, -1] - tab[:, 0]
        sizes = [min(512, n - 512 * c) for c in range(len(nnz))]
        assert sizes == ([512, 512, 6] if n == 1030 else [512, 512, 1])
        assert (nnz[0] > 2560) == (KW == 6), f'{what}: chunk 0 holds {nnz[0]} entries'      # lists read from global memory / staged
        assert bool(u.n == st.V and vp_rows == st.V) == ident
    if special:
        cnt = np.diff(s['jcsr_start'])
        assert cnt[7] == 0 and cnt[3] == n, 'no empty joint / no joint that owns every vertex'
    A, tr = rigid_transforms(B, nj, g), torch.zeros(B, 3)
    vposed = torch.full((B, vp_rows, 3), NAN)
    vposed[:, torch.from_numpy(np.asarray(vp_row)).long()] = torch.randn(B, n, 3, generator=g) * 0.5
    vp_sel = vposed[:, torch.from_numpy(np.asarray(vp_row)).long()]
    dverts = torch.randn(B, n, 3, generator=g)
    Dk3 = torch.from_numpy(s['Dk'][:, :3 * n])
    ref = bwd_reference(sk, ids, A, vp_sel, tr, dverts, Dk3, torch.float64)
    f32 = bwd_reference(sk, ids, A, vp_sel, tr, dverts, Dk3, torch.float32)
    Ad, vpd, dvd = A.to(dev), vposed.to(dev), dverts.to(dev)
    want_dtr = o.get('dtransl', True)
    runs = []
    for rep in range(2 if o.get('twice') else 1):
        bufs = [guarded(B * NCs, dev), guarded(B * nj * 12, dev), guarded(B * 3, dev), guarded(B * K_PAD, dev)]
        (_, dvp), (_, dA), (_, dtr), (_, dX) = bufs
        rc = lib.lbs_verts_bwd(C.byref(st), C.byref(u), ptr(Ad), nj, ptr(vpd), vp_rows, ptr(dvd), B, _roundup(B, 32), ptr(dvp), ptr(dA),
                               ptr(dtr) if want_dtr else None, ptr(dX), lib.stream(dev))
        _sync(lib)
        assert rc == 0, f'{what}: refused ({rc})'
        out = [guards_intact(w, m, f'{what} {k}').clone() for (w, _), m, k in zip(bufs, (B * NCs, B * nj * 12, B * 3, B * K_PAD), ('dvp', 'dA', 'dtransl', 'dX'))]
        for k in ('part', 'gemm_part'):
            if k in ut:
                guards_intact(ut[k + '_whole'], ut[k].numel(), f'{what} {k}')
        runs.append(out)
    dvp, dA, dtr, dX = runs[0]
    dvp = dvp.view(B, NCs)
    assert (dvp[:, 3 * n:].view(torch.int32) == 0).all() if NCs > 3 * n else True, f'{what}: dvp pad columns are not zero'
    fam = f'lbs_bwd {route}'
    gate(fam + ' dvp', dvp[:, :3 * n], f32[0], ref[0], what + ' dvp')
    gate(fam + ' dA', dA.view(B, nj, 12), f32[1], ref[1], what + ' dA')
    if want_dtr:
        gate(fam + ' dtransl', dtr.view(B, 3), f32[2], ref[2], what + ' dtransl')
    else:
        assert torch.isnan(dtr).all(), f'{what}: wrote dtransl although none was asked for'
    gate(fam + ' dX', dX.view(B, K_PAD), f32[3], ref[3], what + ' dX')
    if len(runs) == 2:
        for a, b, k in zip(runs[0], runs[1], ('dvp', 'dA', 'dtransl', 'dX')):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: two launches differ in {k} (the route is documented as order-fixed)'
    ROUTES_RUN.add(route)
    return route


def check_bwd_refusals(lib, dev):
    V, n, nj, KW, B = 40, 30, 55, 4, 2
    g = torch.Generator().manual_seed(3)
    sk = make_skin(V, nj, KW, 3)
    ids = torch.randperm(V, generator=g)[:n].numpy()
    st, keep = skin_const(sk, dev)
    A, vpd, dvd = rigid_transforms(B, nj, g).to(dev), torch.randn(B, V, 3, generator=g).to(dev), torch.randn(B, n, 3, generator=g).to(dev)
    for why, code in (('NCs % 16', ERR_SHAPE), ('NCs < 3 n', ERR_SHAPE), ('n = 0', ERR_SHAPE), ('B = 0', ERR_SHAPE), ('no dverts', ERR_ARG)):
        u, ut, s = vertex_set(sk, ids, None, dev)
        Bc = B
        if why == 'NCs % 16':
            u.NCs = 92
        if why == 'NCs < 3 n':
            u.NCs = 80
        if why == 'n = 0':
            u.n = 0
        if why == 'B = 0':
            Bc = 0
        bufs = [guarded(B * 96, dev), guarded(B * nj * 12, dev), guarded(B * 3, dev), guarded(B * K_PAD, dev)]
        rc = lib.lbs_verts_bwd(C.byref(st), C.byref(u), ptr(A), nj, ptr(vpd), V, None if why == 'no dverts' else ptr(dvd), Bc, 32, ptr(bufs[0][1]),
                               ptr(bufs[1][1]), ptr(bufs[2][1]), ptr(bufs[3][1]), lib.stream(dev))
        _sync(lib)
        assert rc == code, f'{why}: {rc}'
        assert all(torch.isnan(w.cpu()).all() for w, _ in bufs), f'{why}: a refused launch wrote its outputs'


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lemo_joints_assemble: joints [B][nj + n_extra + n_lmk][3], a block of 128 threads strides over (nj + n_extra + n_lmk) * 3 values

JOINT_CASES = ((55, 21, 51, True), (55, 21, 51, False), (55, 0, 51, True), (55, 21, 0, True), (3, 2, 1, False))   # (nj, n_extra, n_lmk, transl)


def check_joints(lib, dev, nj, n_extra, n_lmk, with_transl, B=3, V=97):
    what = f'joints_assemble nj {nj} extra {n_extra} lmk {n_lmk} transl {with_transl}'
    g = torch.Generator().manual_seed(nj + n_extra * 3 + n_lmk * 7)
    Jtr, verts, tr = torch.randn(B, nj, 3, generator=g), torch.randn(B, V, 3, generator=g), torch.randn(B, 3, generator=g)
    extra = torch.randint(V, (max(n_extra, 1),), generator=g).int()
    rows = torch.randint(V, (max(n_lmk, 1), 3), generator=g).int()
    bary = torch.rand(max(n_lmk, 1), 3, generator=g)
    bary = (bary / bary.sum(1, keepdim=True)).contiguous()
    nt = nj + n_extra + n_lmk
    if (nj, n_extra, n_lmk) == (55, 21, 51):
        assert nt * 3 == 381                                # three trips of the 128-thread loop
    whole, out = guarded(B * nt * 3, dev)
    d = lambda t: t.to(dev)
    keep = [d(Jtr), d(verts), d(extra), d(rows), d(bary), d(tr)]
    rc = lib.joints_assemble(ptr(keep[0]), nj, ptr(keep[1]), V, ptr(keep[2]) if n_extra else None, n_extra, ptr(keep[3]) if n_lmk else None,
                             ptr(keep[4]) if n_lmk else None, n_lmk, ptr(keep[5]) if with_transl else None, B, ptr(out), lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    j = guards_intact(whole, B * nt * 3, what).view(B, nt, 3)
    same_bits(j[:, :nj], Jtr + tr[:, None] if with_transl else Jtr, f'{what}: posed joints (one IEEE addition)')
    if n_extra:
        same_bits(j[:, nj:nj + n_extra], verts[:, extra.long()], f'{what}: vertex picks')
    if n_lmk:
        terms = verts[:, rows.long()].double() * bary.double()[None, :, :, None]           # [B][n_lmk][3 corners][3]
        err = (j[:, nj + n_extra:].double() - terms.sum(2)).abs()
        tol = 3 * U * terms.abs().sum(2)
        print(f'{what}: landmark error / bound {float((err / tol).max()):.3f}')
        assert (err <= tol).all(), f'{what}: landmarks off by {float((err / tol).max()):.2f} x 3 * 2^-24 * sum |terms|'


# ---------------------------------------------------------------------------------------------------------------------------
# 5. lemo_rot6d_to_aa_fwd / _bwd: 6-D -> rotation matrix (Gram-Schmidt) -> quaternion (four branches) -> axis-angle, the torchgeometry
#    formulas rot.hpp cites, restated in torch

ROT_N = (1, 64, 65)
ROT_STRIDE = 9


def rot6d_to_matrix(x6):
    """convert_to_3D_rot: columns b1 = normalize(a1), b2 = normalize(a2 - <b1, a2> b1), b3 = b1 x b2"""
    a1, a2 = x6[:, 0::2], x6[:, 1::2]                                   # x6 viewed as [3][2]
    b1 = a1 / a1.norm(dim=1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=1, keepdim=True)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=1)], -1)        # [N][3][3]


def quat_branch(R):
    """torchgeometry.rotation_matrix_to_quaternion's branch on the TRANSPOSED matrix (it is handed R^T): 0 .. 3"""
    Rt = R.transpose(1, 2)
    d2, d0, d1 = Rt[:, 2, 2] < 1e-6, Rt[:, 0, 0] > Rt[:, 1, 1], Rt[:, 0, 0] < -Rt[:, 1, 1]
    return torch.where(d2, torch.where(d0, 0, 1), torch.where(d1, 2, 3))


def branch_margin(R):
    """distance of each row from the nearest branch boundary it can cross: R22 = 1e-6, and R00 = R11 below it, R00 = -R11 above"""
    second = torch.where(R[:, 2, 2] < 1e-6, (R[:, 0, 0] - R[:, 1, 1]).abs(), (R[:, 0, 0] + R[:, 1, 1]).abs())
    return torch.minimum((R[:, 2, 2] - 1e-6).abs(), second)


def matrix_to_aa(R):
    """torchgeometry rotation_matrix_to_angle_axis = quaternion_to_angle_axis(rotation_matrix_to_quaternion(R)), eps 1e-6"""
    Rt = R.transpose(1, 2)
    r = lambda i, j: Rt[:, i, j]
    t0 = 1 + r(0, 0) - r(1, 1) - r(2, 2)
    q0 = torch.stack([r(1, 2) - r(2, 1), t0, r(0, 1) + r(1, 0), r(2, 0) + r(0, 2)], -1)
    t1 = 1 - r(0, 0) + r(1, 1) - r(2, 2)
    q1 = torch.stack([r(2, 0) - r(0, 2), r(0, 1) + r(1, 0), t1, r(1, 2) + r(2, 1)], -1)
    t2 = 1 - r(0, 0) - r(1, 1) + r(2, 2)
    q2 = torch.stack([r(0, 1) - r(1, 0), r(2, 0) + r(0, 2), r(1, 2) + r(2, 1), t2], -1)
    t3 = 1 + r(0, 0) + r(1, 1) + r(2, 2)
    q3 = torch.stack([t3, r(1, 2) - r(2, 1), r(2, 0) - r(0, 2), r(0, 1) - r(1, 0)], -1)
    br = quat_branch(R)
    q = torch.where((br == 0)[:, None], q0, torch.where((br == 1)[:, None], q1, torch.where((br == 2)[:, None], q2, q3)))
    t = torch.where(br == 0, t0, torch.where(br == 1, t1, torch.where(br == 2, t2, t3)))
    q = q * (0.5 / torch.sqrt(t))[:, None]
    s2 = (q[:, 1:] ** 2).sum(1)
    s, c = torch.sqrt(s2), q[:, 0]
    two_theta = 2.0 * torch.where(c < 0.0, torch.atan2(-s, -c), torch.atan2(s, c))
    k = torch.where(s2 > 0.0, two_theta / s, 2.0 * torch.ones_like(s))
    return q[:, 1:] * k[:, None]


def gram_schmidt_sine(x6):
    """|sin| of the angle between a1 and a2.  Gram-Schmidt forms u = a2 - <b1, a2> b1 with |u| = |a2| sin: the rounding of b1 and of the
    dot product reaches b2 magnified by 1 / sin, so two correct float32 evaluations of one nearly parallel row differ from float64 by
    amounts that scatter over that factor (measured on a row with sin 0.27: 1e-7, 4e-7 and 8e-7 for a / |a|, a / n and a * (1 / n)), and
    a gate between two of them measures luck, not the kernel.  The inputs are therefore drawn with sin >= 0.5 (magnification <= 2)."""
    a1, a2 = x6[:, 0::2], x6[:, 1::2]
    return torch.cross(a1, a2, dim=1).norm(dim=1) / (a1.norm(dim=1) * a2.norm(dim=1))


def rot_inputs(N, seed):
    """[N][6] float32 inputs; N >= 64: at least 8 rows in each quaternion branch, every row >= 1e-3 from a branch boundary, and rows at
    rotation angles 1e-4, pi / 2 and pi - 1e-3; every row well conditioned for Gram-Schmidt (gram_schmidt_sine)"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    while len(rows) < N:
        x = (torch.randn(4 * N + 64, 6, generator=g) * torch.rand(4 * N + 64, 1, generator=g).mul(2).add(0.2)).float()
        R = rot6d_to_matrix(x.double())
        ok = (branch_margin(R) >= 1e-3) & (gram_schmidt_sine(x.double()) >= 0.5)
        br = quat_branch(R)
        if N == 1:
            rows = [x[ok][0]]
            break
        per = [x[ok & (br == b)] for b in range(4)]
        assert all(len(p) >= 8 for p in per)
        rows = [p[i] for i in range((N - 3 + 3) // 4 + 1) for p in per][:N - 3]
        for ang in (1e-4, np.pi / 2, np.pi - 1e-3):        # a rotation by `ang` about a generic axis, as its first two columns scaled
            ax = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
            Rm = rigid_from_axis_angle(ax / ax.norm() * ang)
            assert float(branch_margin(Rm[None])) >= 1e-3
            rows.append(torch.stack([Rm[:, 0] * 1.7, Rm[:, 1] * 0.6], 1).reshape(6).float())
    return torch.stack(rows).contiguous()


def rigid_from_axis_angle(aa):
    th = aa.norm()
    k = aa / th
    Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * Kx + (1 - torch.cos(th)) * (Kx @ Kx)


def check_rot6d(lib, dev, N):
    what = f'rot6d_to_aa N {N}'
    x = rot_inputs(N, seed=N)
    R64 = rot6d_to_matrix(x.double())
    if N >= 64:
        cnt = torch.bincount(quat_branch(R64), minlength=4)
        assert (cnt >= 8).all(), f'branch census {cnt.tolist()}'
        ang = matrix_to_aa(R64[-3:]).norm(dim=1)
        assert torch.allclose(ang, torch.tensor([1e-4, np.pi / 2, np.pi - 1e-3], dtype=torch.float64), rtol=1e-3)
    assert (branch_margin(R64) >= 1e-3).all()
    assert torch.equal(quat_branch(R64), quat_branch(rot6d_to_matrix(x))), 'float32 takes another branch'
    xs = torch.full((N, ROT_STRIDE), NAN)
    xs[:, :6] = x
    g = torch.Generator().manual_seed(N + 1)
    d_aa = torch.randn(N, 3, generator=g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        xl = x.to(dtype).requires_grad_(True)
        aa = matrix_to_aa(rot6d_to_matrix(xl))
        dx, = torch.autograd.grad(aa, xl, d_aa.to(dtype))
        res[dtype] = (aa.detach(), dx)
    xd, dd = xs.to(dev), d_aa.to(dev)
    awhole, aa = guarded(N * 3, dev)
    rc = lib.rot6d_to_aa_fwd(ptr(xd), ROT_STRIDE, N, ptr(aa), lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    gate('rot6d_to_aa fwd', guards_intact(awhole, N * 3, what).view(N, 3), res[torch.float32][0], res[torch.float64][0], what + ' fwd')
    gwhole, dx = guarded(N * 6, dev)
    rc = lib.rot6d_to_aa_bwd(ptr(xd), ROT_STRIDE, ptr(dd), N, ptr(dx), lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    gate('rot6d_to_aa bwd', guards_intact(gwhole, N * 6, what).view(N, 6), res[torch.float32][1], res[torch.float64][1], what + ' bwd')


# ---------------------------------------------------------------------------------------------------------------------------
# 4b. lemo_smplx_pose_fwd / _bwd against oracle.lemo_oracle.SmplxOracle in float64 (and its float32 self as the yardstick)

POSE_CASES = ((1, 12, True, 'bf16'), (33, 12, False, 'f16'), (33, 0, True, 'f16'), (1, 0, False, 'bf16'))     # (B, ncomp, expr, XgS form)
POSE_OUT = ('full_pose', 'R', 'J', 'A', 'Jtr')
# backward: (B, ncomp, expr, d_full_pose).  The kernel is one workgroup per frame with no path that depends on B, so B only sets how
# many entries each compared gradient has; the smallest (d_global_orient, d_jaw, d_leye, d_reye: 3 per frame) has 99 at B = 33.  At
# B = 1 the gate would compare the maxima of three (d_expr: ten) rounding errors, which is sampling luck in either direction: a
# first draft with B = 1 met a float32 restatement that was right to 0.14 ulp in all ten d_expr entries, against a kernel right to
# 0.75 ulp (less than blocks_common's floor), and called that a ratio of 5.4.
POSE_BWD_CASES = ((33, 12, True, True), (33, 12, False, False), (33, 0, True, True), (33, 0, False, False))


def pose_model():
    from lemo_amd import synthetic
    return synthetic.make_synthetic_smplx(seed=5, V=64, F=96)


def pose_inputs(B, ncomp, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.4).contiguous()
    hd = ncomp if ncomp else 45
    return dict(go=r(B, 3), body=r(B, 63), jaw=r(B, 3), leye=r(B, 3), reye=r(B, 3), lh=r(B, hd), rh=r(B, hd), betas=r(B, 10) * 2, expr=r(B, 10))


def pose_reference(model, p, ncomp, with_expr, dtype, grads=None):
    """SmplxOracle's pose stage in `dtype` from the float32 inputs -> dict(full_pose, R, J, A, Jtr, X [B][512]); with `grads` =
    (dA, dJtr, dX, d_full_pose or None) also the gradients of sum(dA A + dJtr Jtr + dX X + dfp full_pose) by autograd"""
    from oracle import lemo_oracle as O
    from oracle.f64 import _to_double, default_f64
    import contextlib
    ctx = default_f64() if dtype == torch.float64 else contextlib.nullcontext()
    with ctx:
        so = O.SmplxOracle(model, num_pca_comps=ncomp if ncomp else 12, use_pca=ncomp > 0, extra_joint_ids=[0])
        if dtype == torch.float64:
            _to_double(so)
        q = {k: v.to(dtype).clone().requires_grad_(grads is not None) for k, v in p.items()}
        B = q['go'].shape[0]
        expr = q['expr'] if with_expr else torch.zeros(B, 10, dtype=dtype)
        fp = so.full_pose(q['go'], q['body'], q['lh'], q['rh'], q['jaw'], q['leye'], q['reye'])
        shape = torch.cat([q['betas'], expr], -1)
        _, Jtr, mid = O.lbs(shape, fp, so.v_template, torch.cat([so.shapedirs, so.expr_dirs], -1), so.posedirs, so.J_regressor, so.parents,
                            so.lbs_weights, return_intermediates=True)
        nj = mid['J'].shape[1]
        X = torch.cat([shape, (mid['rot_mats'][:, 1:] - torch.eye(3, dtype=dtype)).reshape(B, -1), torch.zeros(B, K_PAD - 20 - 9 * (nj - 1), dtype=dtype)], 1)
        out = dict(full_pose=fp, R=mid['rot_mats'].reshape(B, nj, 9), J=mid['J'], A=mid['A'][:, :, :3, :].reshape(B, nj, 12), Jtr=Jtr, X=X)
        if grads is None:
            return {k: v.detach() for k, v in out.items()}
        dA, dJtr, dX, dfp = grads
        loss = (out['A'] * dA.to(dtype)).sum() + (out['Jtr'] * dJtr.to(dtype)).sum() + (X * dX.to(dtype)).sum()
        if dfp is not None:
            loss = loss + (fp * dfp.to(dtype)).sum()
        names = [k for k in q if with_expr or k != 'expr']
        gr = torch.autograd.grad(loss, [q[k] for k in names])
        return dict(zip(names, gr))


def _pose_ws(B, nj, dev, f16):
    """a guarded pose workspace: outputs NaN, Xg / XgS zero (their pad entries must stay zero bits)"""
    Bp = _roundup(B, 32)
    sizes = dict(full_pose=B * nj * 3, R=B * nj * 9, J=B * nj * 3, T=B * nj * 12, A=B * nj * 12, Jtr=B * nj * 3)
    w = {k: guarded(m, dev) for k, m in sizes.items()}
    w['Xg'] = guarded(K_PAD // 8 * Bp * 8, dev, fill=0.0)
    nxs = K_PAD // 16 * (2 if f16 else 3) * Bp * 16
    xs_whole = torch.full((nxs + 128,), 0x5A5A, dtype=torch.int16, device=dev)
    xs_whole[64:64 + nxs] = 0
    w['XgS'] = (xs_whole, xs_whole[64:64 + nxs])
    ws = _hip.PoseWs(*[ptr(w[k][1]) for k in ('full_pose', 'R', 'J', 'T', 'A', 'Jtr', 'Xg')], Bp, ptr(w['XgS'][1]), 1 if f16 else 0)
    return ws, w, Bp, dict(sizes, Xg=K_PAD // 8 * Bp * 8)


def _pose_results(w, sizes, B, nj, Bp, f16, what):
    out = {k: guards_intact(w[k][0], sizes[k], f'{what} {k}').clone() for k in sizes}
    xs_whole, xs = w['XgS'][0].cpu(), w['XgS'][1].cpu()
    assert (xs_whole[:64] == 0x5A5A).all() and (xs_whole[64 + xs.numel():] == 0x5A5A).all(), f'{what}: wrote outside XgS'
    out['XgS'] = xs.view(K_PAD // 16, 2 if f16 else 3, Bp, 2, 8).clone()
    return out


def run_pose_fwd(lib, dev, db, p, B, with_expr, f16, what, rot6d=None, vposer_o=None):
    nj = db.data.nj
    ws, w, Bp, sizes = _pose_ws(B, nj, dev, f16)
    d = {k: v.to(dev) for k, v in p.items()}
    hd = p['lh'].shape[1]
    pin = _hip.PoseIn(ptr(d['go']), ptr(d['body']), ptr(d['jaw']), ptr(d['leye']), ptr(d['reye']), ptr(d['lh']), ptr(d['rh']), hd, ptr(d['betas']), 10,
                      ptr(d['expr']) if with_expr else None)
    keep = [d]
    if rot6d is not None:                                  # the fused producers replace global_orient / body_pose: those hold NaN
        r6, vo = rot6d.to(dev), vposer_o.to(dev)
        d['go'].fill_(NAN), d['body'].fill_(NAN)
        gwhole, go_out = guarded(B * 3, dev)
        pin.rot6d, pin.vposer_o, pin.go_out = ptr(r6), ptr(vo), ptr(go_out)
        keep += [r6, vo, gwhole]
    rc = lib.smplx_pose_fwd(C.byref(db.body), C.byref(pin), C.byref(ws), B, lib.stream(dev))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    out = _pose_results(w, sizes, B, nj, Bp, f16, what)
    if rot6d is not None:
        out['go_out'] = guards_intact(gwhole, B * 3, what + ' go_out').view(B, 3).clone()
    return out, ws, w, Bp


def check_pose_fwd(lib, dev, B, ncomp, with_expr, form):
    from lemo_amd.body_model import DeviceBody
    what = f'smplx_pose_fwd B {B} ncomp {ncomp} expr {with_expr} XgS {form}'
    model, f16 = pose_model(), form == 'f16'
    data = BodyModelData(model, num_pca_comps=ncomp if ncomp else 12, use_pca=ncomp > 0)
    db = DeviceBody(data, dev, blend_f16=f16)
    nj = data.nj
    p = pose_inputs(B, ncomp, seed=B * 10 + ncomp)
    ref, f32 = pose_reference(model, p, ncomp, with_expr, torch.float64), pose_reference(model, p, ncomp, with_expr, torch.float32)
    out, _, _, Bp = run_pose_fwd(lib, dev, db, p, B, with_expr, f16, what)
    shapes = dict(full_pose=(B, nj * 3), R=(B, nj, 9), J=(B, nj, 3), A=(B, nj, 12), Jtr=(B, nj, 3))
    for k in POSE_OUT:
        gate(f'smplx_pose_fwd {k}', out[k].view(shapes[k]), f32[k], ref[k], f'{what} {k}')
    Xg = out['Xg'].view(K_PAD // 8, Bp, 8)
    gate('smplx_pose_fwd Xg', Xg[:, :B].permute(1, 0, 2).reshape(B, K_PAD), f32['X'], ref['X'], what + ' Xg')
    nfeat = 20 + 9 * (nj - 1)
    flat = Xg.permute(1, 0, 2).reshape(Bp, K_PAD)
    assert (flat[B:].view(torch.int32) == 0).all() and (flat[:, nfeat:].view(torch.int32) == 0).all(), f'{what}: Xg pad entries are not zero bits'
    xg16 = Xg.view(-1, 2, Bp, 8).permute(0, 2, 1, 3).double()                             # [K/16][Bp][2][8]
    if f16:
        back = out['XgS'].view(torch.float16).double().sum(1)
        assert float((back - xg16).abs().max()) <= float(xg16.abs().max()) * 2.0 ** -21, f'{what}: fp16 XgS misses Xg by more than 2^-21 max'
    else:
        back = ((out['XgS'].to(torch.int32) & 0xFFFF) << 16).view(torch.float32).double().sum(1)
        assert torch.equal(back, xg16), f'{what}: the three bf16 pieces do not resum to Xg'
    xs = out['XgS'].permute(2, 0, 3, 4, 1).reshape(Bp, K_PAD, -1)                          # [frame][feature][piece]
    assert (xs[B:] == 0).all() and (xs[:, nfeat:] == 0).all(), f'{what}: XgS pad entries are not zero bits'
    assert float(xg16.abs().max()) > 0.1


def check_pose_fused_producers(lib, dev, B):
    """rot6d / vposer_o inside the pose kernel == the axis-angles of lemo_rot6d_to_aa_fwd fed as global_orient / body_pose: equal bits"""
    from lemo_amd.body_model import DeviceBody
    what = f'smplx_pose_fwd fused producers B {B}'
    data = BodyModelData(pose_model())
    db = DeviceBody(data, dev, blend_f16=True)
    p = pose_inputs(B, 12, seed=B)
    g = torch.Generator().manual_seed(B + 77)
    rot6d = torch.randn(B, 6, generator=g).contiguous()
    vo = torch.full((B, 128), NAN)
    vo[:, :126] = torch.randn(B, 126, generator=g)
    r6d, vod = rot6d.to(dev), vo.to(dev)
    awhole, go = guarded(B * 3, dev)
    bwhole, body = guarded(B * 63, dev)
    assert lib.rot6d_to_aa_fwd(ptr(r6d), 6, B, ptr(go), lib.stream(dev)) == 0
    for b in range(B):
        assert lib.rot6d_to_aa_fwd(ptr(vod[b]), 6, 21, ptr(body.view(B, 63)[b]), lib.stream(dev)) == 0
    _sync(lib)
    q = dict(p, go=guards_intact(awhole, B * 3, what).view(B, 3).clone(), body=guards_intact(bwhole, B * 63, what).view(B, 63).clone())
    assert torch.isfinite(q['go']).all() and torch.isfinite(q['body']).all()
    plain, _, _, _ = run_pose_fwd(lib, dev, db, q, B, True, True, what + ' (axis-angles)')
    fused, _, _, _ = run_pose_fwd(lib, dev, db, p, B, True, True, what, rot6d=rot6d, vposer_o=vo)
    same_bits(fused['go_out'], q['go'], f'{what}: go_out')
    for k in POSE_OUT + ('Xg',):
        same_bits(fused[k], plain[k], f'{what}: {k}')
    assert torch.equal(fused['XgS'], plain['XgS']), f'{what}: XgS'


def check_pose_bwd(lib, dev, B, ncomp, with_expr, with_dfp):
    from lemo_amd.body_model import DeviceBody
    what = f'smplx_pose_bwd B {B} ncomp {ncomp} expr {with_expr} d_full_pose {with_dfp}'
    model = pose_model()
    data = BodyModelData(model, num_pca_comps=ncomp if ncomp else 12, use_pca=ncomp > 0)
    db = DeviceBody(data, dev, blend_f16=True)
    nj = data.nj
    p = pose_inputs(B, ncomp, seed=B * 10 + ncomp + 1)
    g = torch.Generator().manual_seed(B + ncomp)
    dA, dJtr, dX = torch.randn(B, nj, 12, generator=g), torch.randn(B, nj, 3, generator=g), torch.zeros(B, K_PAD)
    dX[:, :20 + 9 * (nj - 1)] = torch.randn(B, 20 + 9 * (nj - 1), generator=g)
    dfp = torch.randn(B, nj * 3, generator=g) if with_dfp else None
    ref = pose_reference(model, p, ncomp, with_expr, torch.float64, (dA, dJtr, dX, dfp))
    f32 = pose_reference(model, p, ncomp, with_expr, torch.float32, (dA, dJtr, dX, dfp))
    _, ws, w, _ = run_pose_fwd(lib, dev, db, p, B, with_expr, True, what + ' (forward)')
    hd = p['lh'].shape[1]
    names = ('go', 'body', 'jaw', 'leye', 'reye', 'lh', 'rh', 'betas', 'expr')
    bufs = {k: guarded(p[k].numel(), dev) for k in names}
    keep = [t.to(dev) for t in (dA, dJtr, dX)] + ([dfp.to(dev)] if with_dfp else [])
    gi = _hip.PoseGradIn(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]) if with_dfp else None)
    go = _hip.PoseGradOut(*[ptr(bufs[k][1]) for k in names[:7]], hd, ptr(bufs['betas'][1]), ptr(bufs['expr'][1]) if with_expr else None)
    rc = lib.smplx_pose_bwd(C.byref(db.body), C.byref(ws), C.byref(gi), C.byref(go), B, lib.stream(dev))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    for k in names:
        got = guards_intact(bufs[k][0], p[k].numel(), f'{what} d_{k}').view(p[k].shape)
        if k == 'expr' and not with_expr:
            assert torch.isnan(got).all(), f'{what}: wrote d_expr although none was asked for'
            continue
        gate(f'smplx_pose_bwd d_{k}', got, f32[k], ref[k], f'{what} d_{k}')


# ---------------------------------------------------------------------------------------------------------------------------
# 5b. the rotation part of lemo_vposer_decode_fwd / _bwd.  The MLP is made a selector: z = s e_k (s > 0) passes through fc1 and fc2
#     unchanged (identity blocks, zero bias: one product with 1 and zeros) and the out layer's column k holds 21 chosen 6-D rows, so
#     o[b] = s_b * W3[:, k_b] is known on the host to the bit and the branch census can be taken before the launch.

VPOSER_B = (1, 33)


def vposer_selector(B, seed):
    rows = rot_inputs(32 * 21, seed)                                   # every branch, the three special angles, margins checked
    W3 = torch.zeros(128, 512)
    W3[:126, :32] = rows.view(32, 126).t()
    W1, W2 = torch.zeros(512, 32), torch.zeros(512, 512)
    W1[:32] = torch.eye(32)
    W2[:32, :32] = torch.eye(32)
    g = torch.Generator().manual_seed(seed + 1)
    z = torch.zeros(B, 32)
    k = (torch.arange(B) * 7 + 3) % 32
    z[torch.arange(B), k] = torch.rand(B, generator=g) + 0.5
    o = torch.zeros(B, 128)
    o[:, :126] = (W3[:126, k] * z[torch.arange(B), k]).t()            # one float32 product per entry
    return (W1, W2, W3), z, o


def check_vposer_rot(lib, dev, B):
    what = f'vposer_decode rotation part B {B}'
    (W1, W2, W3), z, o_want = vposer_selector(B, seed=B + 40)
    x6 = o_want[:, :126].reshape(B * 21, 6)
    R64 = rot6d_to_matrix(x6.double())
    assert (branch_margin(R64) >= 1e-3).all() and torch.equal(quat_branch(R64), quat_branch(rot6d_to_matrix(x6)))
    if B > 1:
        assert (torch.bincount(quat_branch(R64), minlength=4) >= 8).all()
    d = lambda t: t.contiguous().to(dev)
    zero512, zero128 = torch.zeros(512), torch.zeros(128)
    keep = [d(W1), d(W1.t()), d(zero512), d(W2), d(W2.t()), d(zero512), d(W3), d(W3.t()), d(zero128)]
    w = _hip.VPoserW(*[ptr(t) for t in keep])
    zd = d(z)
    h1w, h1 = guarded(B * 512, dev)
    h2w, h2 = guarded(B * 512, dev)
    ow, o = guarded(B * 128, dev)
    mw, matrot = guarded(B * 21 * 9, dev)
    aw, aa = guarded(B * 63, dev)
    rc = lib.vposer_decode_fwd(C.byref(w), ptr(zd), 32, B, ptr(h1), ptr(h2), ptr(o), ptr(matrot), ptr(aa), lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    same_bits(guards_intact(ow, B * 128, what + ' o').view(B, 128) + 0.0, o_want, f'{what}: the selector MLP did not hand the chosen rows through')
    g = torch.Generator().manual_seed(B)
    d_aa, d_mat = torch.randn(B * 21, 3, generator=g), torch.randn(B * 21, 3, 3, generator=g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        xl = x6.to(dtype).requires_grad_(True)
        R = rot6d_to_matrix(xl)
        a = matrix_to_aa(R)
        res[dtype] = (R.detach(), a.detach(), torch.autograd.grad(a, xl, d_aa.to(dtype), retain_graph=True)[0],
                      torch.autograd.grad(R, xl, d_mat.to(dtype), retain_graph=True)[0],
                      torch.autograd.grad((a * d_aa.to(dtype)).sum() + (R * d_mat.to(dtype)).sum(), xl)[0])
    r64, r32 = res[torch.float64], res[torch.float32]
    gate('vposer_rot fwd matrot', guards_intact(mw, B * 189, what + ' matrot').view(B * 21, 3, 3), r32[0], r64[0], what + ' matrot')
    gate('vposer_rot fwd aa', guards_intact(aw, B * 63, what + ' aa').view(B * 21, 3), r32[1], r64[1], what + ' aa')
    dad, dmd = d(d_aa), d(d_mat)
    for i, (use_aa, use_mat) in enumerate(((True, False), (False, True), (True, True))):
        sw, scratch = guarded(B * 1152, dev)
        zw, dz = guarded(B * 32, dev)
        rc = lib.vposer_decode_bwd(C.byref(w), ptr(h1), ptr(h2), ptr(o), ptr(dad) if use_aa else None, ptr(dmd) if use_mat else None, B, ptr(dz), 32,
                                   ptr(scratch), lib.stream(dev))
        _sync(lib)
        assert rc == 0, rc
        guards_intact(zw, B * 32, what + ' dz')
        dout = guards_intact(sw, B * 1152, what + ' scratch')[:B * 128].view(B, 128)
        assert (dout[:, 126:].view(torch.int32) == 0).all(), f'{what}: d(out) pad entries are not zero'
        gate('vposer_rot bwd', dout[:, :126].reshape(B * 21, 6), r32[2 + i], r64[2 + i], f'{what} d(out) aa {use_aa} matrot {use_mat}')
    whole, dz = guarded(B * 32, dev)                                   # neither gradient: refused, nothing written
    assert lib.vposer_decode_bwd(C.byref(w), ptr(h1), ptr(h2), ptr(o), None, None, B, ptr(dz), 32, ptr(scratch), lib.stream(dev)) == ERR_ARG
    _sync(lib)
    assert torch.isnan(whole.cpu()).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the pose kernel's own XgS feeding lbs_verts_fwd_xs on a synthetic SMPL-X-shaped model (V = 200, B = 5; formerly in test_kernels_emu.py)

def _model_pose_run(lib, dev, f16, seed=1):
    """BodyModelData / DeviceBody of the synthetic model, one lemo_smplx_pose_fwd -> (data, db, tt, Bp, B, transl)"""
    from lemo_amd import synthetic
    from lemo_amd.body_model import DeviceBody, alloc_pose_ws
    data = BodyModelData(synthetic.make_synthetic_smplx(seed=3, V=200, F=300))
    db = DeviceBody(data, dev, blend_f16=f16)
    B = 5
    ws, tt, Bp = alloc_pose_ws(B, data.nj, dev, f16)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).contiguous().to(dev)
    go, body, lh, rh, betas = r(B, 3), r(B, 63), r(B, 12), r(B, 12), r(B, 10)
    z3, expr, tr = torch.zeros(B, 3).to(dev), r(B, 10), r(B, 3)
    pin = _hip.PoseIn(ptr(go), ptr(body), ptr(z3), ptr(z3), ptr(z3), ptr(lh), ptr(rh), 12, ptr(betas), 10, ptr(expr))
    lib.check(lib.smplx_pose_fwd(C.byref(db.body), C.byref(pin), C.byref(ws), B, lib.stream(dev)))
    _sync(lib)
    return data, db, tt, Bp, B, tr


def check_presplit_blend_bits(lib, dev):
    """lemo_lbs_verts_fwd_xs (per-frame features pre-split into bf16 pieces by the pose kernel, lemo_pose_ws.XgS) against
    lemo_lbs_verts_fwd (every workgroup converts them itself): same pieces, same products in the same order -> same bits;
    and XgS really is the exact 3-way split of Xg"""
    data, db, tt, Bp, B, _ = _model_pose_run(lib, dev, False)
    # XgS[k >> 4][piece][frame][(k >> 3) & 1][k & 7] (bf16 bits) sums back to Xg[k >> 3][frame][k & 7] exactly
    pieces = (tt['XgS'].cpu().to(torch.int32) & 0xFFFF) << 16
    xs = pieces.view(torch.float32).double().sum(1)                                      # [K/16][Bp][2][8]
    xg = tt['Xg'].cpu().view(-1, 2, Bp, 8).permute(0, 2, 1, 3).double()                  # [K/16][Bp][2][8]
    assert torch.equal(xs, xg) and float(xg.abs().max()) > 0
    out = []
    for pre in (False, True):
        v, vp = torch.empty(B, data.V, 3, device=dev), torch.empty(B, data.V, 3, device=dev)
        if pre:
            lib.check(lib.lbs_verts_fwd_xs(C.byref(db.skin), ptr(tt['Xg']), ptr(tt['XgS']), Bp, ptr(tt['A']), data.nj, None, None, data.V, B,
                                           ptr(v), ptr(vp), lib.stream(dev)))
        else:
            lib.check(lib.lbs_verts_fwd(C.byref(db.skin), ptr(tt['Xg']), Bp, ptr(tt['A']), data.nj, None, None, data.V, B, ptr(v), ptr(vp),
                                        lib.stream(dev)))
        _sync(lib)
        out.append((v.cpu(), vp.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0].abs().max()) > 0


def check_f16_presplit_blend(lib, dev):
    """the blend GEMM with BOTH operands pre-split into two fp16 pieces (lemo_skin_const.DgH made on the host, XgS written in its
    fp16 form by the pose kernel; 3 fp16 MFMA products per k-chunk) against a float64 evaluation of the same blend + skinning:
    gated against the float32 restatement (plus the fp16 operand term), inside 4e-7 of the scale, and -- as an extra, as before -- the
    error of the exact three-piece bf16 form on the same model to within a small factor; the pieces carry their operands to 2^-22; ragged
    frame count, all vertices and a vertex subset"""
    res = {}
    for f16 in (True, False):
        data, db, tt, Bp, B, tr = _model_pose_run(lib, dev, f16)
        if f16:
            h, inv = split_f16_pairs(data.Dg)
            hp = h.view(np.float16).reshape(data.Dg.shape[0], data.Dg.shape[1], 2, 2, 4).astype(np.float64)
            back = (hp[:, :, :, 0, :] + hp[:, :, :, 1, :]).reshape(data.Dg.shape) * inv
            assert np.abs(back - data.Dg).max() <= np.abs(data.Dg).max() * 2.0 ** -21
        assert (db.skin.DgH is not None) == f16
        Xgc = tt['Xg'].cpu()
        if f16:                                            # XgS[k >> 4][piece][frame][half][8] (fp16 bits) sums back to Xg to 2^-22
            pc = tt['XgS'].cpu().view(torch.float16).double().sum(1)
            xg = Xgc.view(-1, 2, Bp, 8).permute(0, 2, 1, 3).double()
            assert float((pc - xg).abs().max()) <= float(xg.abs().max()) * 2.0 ** -21 and float(xg.abs().max()) > 0.1
        v, vp = torch.empty(B, data.V, 3, device=dev), torch.empty(B, data.V, 3, device=dev)
        lib.check(lib.lbs_verts_fwd_xs(C.byref(db.skin), ptr(tt['Xg']), ptr(tt['XgS']), Bp, ptr(tt['A']), data.nj, ptr(tr), None,
                                       data.V, B, ptr(v), ptr(vp), lib.stream(dev)))
        ids = torch.arange(3, data.V, 7, dtype=torch.int32)
        idd = ids.to(dev)
        vs = torch.empty(B, len(ids), 3, device=dev)
        lib.check(lib.lbs_verts_fwd_xs(C.byref(db.skin), ptr(tt['Xg']), ptr(tt['XgS']), Bp, ptr(tt['A']), data.nj, ptr(tr), ptr(idd),
                                       len(ids), B, ptr(vs), None, lib.stream(dev)))
        _sync(lib)
        v, vp, vs = v.cpu(), vp.cpu(), vs.cpu()
        assert torch.equal(vs, v[:, ids.long()])
        # float64 reference (and the float32 restatement) from the kernel's own inputs: Xg features, D, A, skinning weights
        X = Xgc.permute(1, 0, 2).reshape(Bp, -1)[:B].contiguous()                         # [B][512]
        sk = types.SimpleNamespace(V=data.V, nj=data.nj, D=data.D, Dg=data.Dg, v_template=data.v_template, w_idx=data.w_idx, w_val=data.w_val)
        A, trc = tt['A'].cpu().reshape(B, data.nj, 3, 4), tr.cpu()
        ref, vpr, T = lbs_reference(sk, X, A, trc, torch.arange(data.V), torch.float64)
        f32_v, f32_p, _ = lbs_reference(sk, X, A, trc, torch.arange(data.V), torch.float32)
        ev, ep = f16_terms(sk, X, T, None, ref, vpr) if f16 else (0.0, 0.0)
        name = 'f16' if f16 else 'bf16_xs'
        gate_plus(f'lbs_fwd {name} verts', v, f32_v, ref, f'model V 200 B 5 {name} verts', ev)
        gate_plus(f'lbs_fwd {name} v_posed', vp, f32_p, vpr, f'model V 200 B 5 {name} v_posed', ep)
        res[f16] = (float((v.double() - ref).abs().max()), float((vp.double() - vpr).abs().max()), float(ref.abs().max()))
    (e16, p16, scale), (e32, p32, _) = res[True], res[False]
    assert e16 < 4e-7 * max(1.0, scale) and p16 < 4e-7 * max(1.0, scale), res
    assert e16 < 4 * e32 + 1e-7 and p16 < 4 * p32 + 1e-7, res
