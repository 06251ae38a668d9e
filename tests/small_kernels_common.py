"""Direct tests of four small kernel families through their own C entry points, against high-precision references on the CPU
(tests/test_small_kernels_emu.py on the host-emulated build, tests/test_small_kernels_gpu.py on the MI355X; both run the cases below):

  lemo_local_markers_4chan, lemo_reconstruct_global_body(_dev), lemo_decode_clip     marker encode / decode   csrc/marker_kernels.hip
  lemo_smooth_loss (smooth_loss_body: also the yardstick of the turn-kernel test)    latent smoothness        csrc/loss_device.hpp
  lemo_adam_flat, lemo_adam_flat_ctr (adam_update_torch, adam_coef_t)                the element update       csrc/common.hpp
  lemo_dec_end_fwd                                                                   decoder end              csrc/prior_train_kernels.hip

A reference is never another kernel; every reference starts from the same float32 inputs.  Below u = 2^-24.

Buffers: every output sits between NaN guards (blocks_common.guarded) and is pre-filled with NaN; every input region the contract
says is not read holds NaN (the last contact row of the encode, the reference slot of reconstruct's input, the pelvis rows and the
unused statistics of decode, the CG8P border of the smoothness input, the gap between dec_end's images); a refused call writes
nothing.  The borders of dec_end's r1 / rec are the caller's zeros and must still be zeros.

1. Marker kernels
-----------------
The kernels compute in float64 and round once to float32.  The reference (`encode_ref`, `reconstruct_ref`, `decode_ref`) restates
them in np.longdouble (>= 63 mantissa bits, asserted): angles by cumsum, translations by cumsum of the rotated steps, the
'nearest'-mode Gaussian filter (sigma 20, radius 80), the heading quaternion.  oracle/markers_oracle.py (sequential quaternion
products in float64, 1e-10-perturbed rotation axis) stays as a CROSS-CHECK of the restatement, within 1e-9 S; it was measured up to
1.8e-10 S from the long-double result at T = 256, S ~ 2, i.e. ~3000 times the bound below: it is too noisy to be the reference of
reconstruct_global_body.
  Bound: every output element obeys |got - ref| <= u |ref| + 2^-40 S, S = max |ref| of that output (per channel for the 4-channel
image).  u |ref| is the one rounding to float32; 2^-40 S covers the <= 256-term float64 scans (a log-step scan adds 8 times per
element, a sequential one 255 times: at most 2^-53 * 256 * the largest partial sum, itself of size S) and the device sin / cos / atan2 /
exp, a few ulp of float64 each: together about 2^-43 S.  rot_0_pivot (a double) is within 2^-48 of the reference.
  Exact parts: the encode's contact columns equal contact[:T-1] bit for bit; channels 1..3 repeat one value over d: all d copies have
equal bits; the third coordinate of reconstruct / decode (post == NULL) equals its input bits; _dev and host-pivot reconstruct give
equal bits; decode labels are exactly (x > 0): sigmoid(0) = 0.5 is not > 0.5.
  Encode inputs: a walking, turning body (heading a random walk, direction markers 27 / 57 / 28 / 58 about 0.3 m apart plus noise),
one case whose heading passes beyond pi / 2.  Quaternions.between is ill-conditioned at -1: before the launch every frame's
across-vector norm must be > 0.1 and the filtered forward direction must have z >= -0.9 (a condition on the inputs).
  decode_clip's reference keeps the float32 stores the kernel documents and the reference code performs (vx, vz, the angle increment
and every de-normalised coordinate are float64 expressions rounded to float32, formed in np.float64 like numpy) and continues in long
double.  With `post` (shift 0.37, a rotation that is not axis-aligned, |t| = 2) the float32 affine map is applied, in float64, to the
kernel's own post == NULL output (the shift as the one float32 addition it is): three products and three additions, each within u of
a quantity <= sum |terms|: 4 u sum |terms| per component, plus the bound above propagated through |M|.

2. lemo_smooth_loss
-------------------
Reference: the float64 stencil (it is turn_common.stencil64's, with the kernel's float32 slope 0.2f; the two are compared).
  dpre, elementwise: |got - ref| <= 4 u |coef2| g (|c - l| [x >= 1] + |r - c| [x <= W - 2]), g = lrelu' from the output: the two
differences are within u |c - l| and u |r - c|, their sum within u |sum| <= u (|c - l| + |r - c|), and the two products add u each.
  Sum of squares: |sum(partial) - sum of float64 squares| <= 32 u sum of squares (sum(partial) taken in float64): all terms are
non-negative, and one block's float32 sum passes about 2 (difference, square) + 16 (4 items x 4 lanes) + 6 (wave butterfly) + 4 (waves)
roundings.
  (1, 1, 8) has no pair: dpre and the sum are exactly 0.  lemo_smooth_loss_blocks == ceil(2 H W (C / 8) / 1024).

3. Adam
-------
Reference: torch.optim.Adam(lr, foreach=False) on the CPU in float32, jumped to step t by planting {step: t - 1, exp_avg, exp_avg_sq}.
  exp_avg, exp_avg_sq: equal bits with torch.  Parameter: |p - p_torch| <= 2 u max(|p_old|, |p_new|) + 6 u |delta|, delta the float64
update formed from the (bit-equal) moments: each side forms delta with three roundings (sqrt / bc2 (+ eps), step * m, the quotient) and
adds with one rounding of a number <= max(|p_old|, |p_new|) (1 + u).  The share of bit-equal parameters is printed and recorded, not
asserted (the device pow may move a coefficient by a float ulp), and so is the share equal to `adam_ops32`, common.hpp's update in
numpy float32 with the host's coefficients: that one tells a device difference from a difference of torch's CPU kernels (torch's
vectorised addcdiv is not the scalar order on every CPU: a host gave 0.90 .. 1.00 against torch where kernel and numpy agreed in
every bit).

4. lemo_dec_end_fwd
-------------------
Reference: float64 F.conv_transpose2d(padding 1).  r1 from u and rec from the kernel's OWN r1 (the second layer is judged alone), both
by conv_shapes_common.check_close(..., 'fp32') with mag = |in| (*) |w| + |b|.

The worst ratio of a measured error to its bound is kept per family in RATIOS and printed by the last test of either module
(DESIGN.md quotes them)."""
import numpy as np
import torch
import torch.nn.functional as F

from blocks_common import GATE, RATIOS, U, _sync, guarded, guards_intact, same_bits           # noqa: F401 (GATE: same yardsticks)
from conv_shapes_common import TAU, check_close, sentinel_cg8p
from lemo_amd._hip import ptr
from oracle import markers_oracle as MO
from turn_common import stencil64

ERR_SHAPE = 10001
ERR_ARG = 10002
NAN = float('nan')
LD = np.longdouble
SLOPE32 = float(np.float32(0.2))                 # LEMO_LRELU_SLOPE as the kernels hold it


SHARE = 'adam bit-equal parameter share'    # RATIOS[SHARE] = (1 - the least share of a (t, lr) case, that share, cases)
SHARE_OPS = 'adam parameter share equal to the float32 restatement'
FAMILIES = set()                             # what this module put into the shared RATIOS


def record(family, ratio, err=0.0):
    r, e, n = RATIOS.get(family, (0.0, 0.0, 0))
    RATIOS[family] = (max(r, float(ratio)), max(e, float(err)), n + 1)
    FAMILIES.add(family)


def report_ratios():
    for k in sorted(FAMILIES):
        r, e, n = RATIOS[k]
        if k in (SHARE, SHARE_OPS):
            print(f'small-kernel {k}: at least {e:.4f} in every (t, lr) case ({n} cases)')
        else:
            print(f'small-kernel ratio {k}: worst measured / bound {r:.3f} (worst error {e:.3e}, {n} comparisons)')
    assert FAMILIES, 'no case ran before the report'


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def guarded_pivot(dev):
    """(whole, view): one double between two runs of 64 NaN doubles, itself NaN"""
    whole = torch.full((129,), NAN, dtype=torch.float64, device=dev)
    return whole, whole[64:65]


def pivot_result(whole, what):
    w = whole.cpu().numpy()
    assert np.isnan(w[:64]).all() and np.isnan(w[65:]).all(), f'{what}: wrote around rot_0_pivot'
    return w[64]


def marker_bound(family, got, ref, what, S=None):
    """|got - ref| <= u |ref| + 2^-40 S in long double; returns the worst ratio"""
    assert np.finfo(LD).nmant >= 63, 'np.longdouble is not an extended format here'
    got = np.asarray(got)
    assert np.isfinite(got).all(), f'{what}: unwritten or non-finite outputs'
    ref = np.asarray(ref, LD)
    S = np.abs(ref).max() if S is None else S
    bound = LD(U) * np.abs(ref) + LD(2.0) ** -40 * S
    err = np.abs(got.astype(LD) - ref)
    ratio = float((err / bound).max()) if bound.min() > 0 else (0.0 if err.max() == 0 else float('inf'))
    record(family, ratio, float(err.max()))
    print(f'{what}: worst |got - ref| / (u |ref| + 2^-40 S) = {ratio:.4f}')
    assert ratio <= 1.0, f'{what}: {ratio:.4f} x the bound at {np.unravel_index(int((err / bound).argmax()), err.shape)}'
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# 1a. lemo_local_markers_4chan

ENC_T = (2, 3, 64, 65, 81, 161, 255, 256)        # 2: one output frame; 64 / 65: a wave; 81 / 161: one / both clamps of the radius-80 filter
MARKER_M1 = (59, 68, 84)                         # inactive; 255 / 256: a ragged and a full block of the scans.  M1 = 59: the smallest body
SDR_L, SDR_R, HIP_L, HIP_R = 27, 57, 28, 58


def encode_inputs(T, M1, wide, seed):
    """a walking, turning body [T, M1, 3] float32 and contact [T, 4] (last row NaN: never read)"""
    rng = np.random.default_rng(seed)
    h = np.cumsum(rng.normal(0, 0.015 if wide else 0.03, T)) + (0.9 + 1.0 * np.arange(T) / T if wide else rng.uniform(-0.5, 0.5))
    step = rng.normal(0.012, 0.004, T)
    pel = np.stack([np.cumsum(-np.sin(h) * step) + 0.3, np.cumsum(np.cos(h) * step) - 0.2, 0.9 + rng.normal(0, 0.01, T)], -1)
    body = pel[:, None] + rng.normal(0, 0.3, (T, M1, 3))
    body[:, 0] = pel
    ac = np.stack([np.cos(h), np.sin(h), np.zeros(T)], -1)                       # across; forward = (-sin h, cos h)
    for row, sgn, up in ((SDR_L, -1, 0.5), (SDR_R, 1, 0.5), (HIP_L, -1, 0.0), (HIP_R, 1, 0.0)):
        body[:, row] = pel + sgn * 0.15 * ac + [0, 0, up] + rng.normal(0, 0.01, (T, 3))
    contact = rng.uniform(-1, 1, (T, 4)).astype(np.float32)
    contact[rng.random((T, 4)) < 0.5] = 1.0
    contact[0, 0] = -0.0
    contact[T - 1] = NAN
    return body.astype(np.float32), contact


def gauss_weights():
    k = np.arange(-80, 81).astype(LD)
    w = np.exp(LD(-0.5) * k * k / LD(400))
    return w / w.sum()


def encode_ref(body, contact):
    """(image [4, T-1, 3 M1 + 4], rot_0_pivot, across norms, filtered forward z) in long double from the float32 inputs"""
    b = body.astype(LD)
    T, M1 = b.shape[:2]
    floor = b[:, :, 2].min()
    ac = (b[:, SDR_R] - b[:, SDR_L]) + (b[:, HIP_R] - b[:, HIP_L])
    n = np.sqrt((ac ** 2).sum(-1))
    fx, fz = -(ac[:, 1] / n), ac[:, 0] / n
    gx, gz = np.zeros(T, LD), np.zeros(T, LD)
    for w, k in zip(gauss_weights(), range(-80, 81)):
        idx = np.clip(np.arange(T) + k, 0, T - 1)
        gx += w * fx[idx]
        gz += w * fz[idx]
    gn = np.sqrt(gx * gx + gz * gz)
    gx, gz = gx / gn, gz / gn
    qw, qy = np.sqrt(gx * gx + gz * gz) + gz, -gx
    qn = np.sqrt(qw * qw + qy * qy)
    qw, qy = qw / qn, qy / qn
    c, s = qw * qw - qy * qy, 2 * qw * qy
    d, Tm = 3 * M1 + 4, T - 1
    img = np.zeros((4, Tm, d), LD)
    x, y = b[:Tm, :, 0] - b[:Tm, :1, 0], b[:Tm, :, 1] - b[:Tm, :1, 1]
    loc = np.stack([c[:Tm, None] * x + s[:Tm, None] * y, -s[:Tm, None] * x + c[:Tm, None] * y, b[:Tm, :, 2] - floor], -1)
    img[0, :, :3 * M1] = loc.reshape(Tm, 3 * M1)
    img[0, :, 3 * M1:] = contact[:Tm].astype(LD)
    vx, vy = b[1:, 0, 0] - b[:-1, 0, 0], b[1:, 0, 1] - b[:-1, 0, 1]
    img[1] = (c[1:] * vx + s[1:] * vy)[:, None]
    img[2] = (-s[1:] * vx + c[1:] * vy)[:, None]
    pw, py = qw[1:] * qw[:-1] + qy[1:] * qy[:-1], qy[1:] * qw[:-1] - qw[1:] * qy[:-1]
    img[3] = np.arctan2(2 * pw * py, pw * pw - py * py)[:, None]
    return img, np.arctan2(2 * qw[0] * qy[0], qw[0] * qw[0] - qy[0] * qy[0]), n, gz


def check_encode(lib, dev, T, M1, wide=False):
    what = f'local_markers_4chan T {T} M1 {M1}' + (' wide' if wide else '')
    body, contact = encode_inputs(T, M1, wide, seed=1000 * T + M1 + (7 if wide else 0))
    ref, piv, n, gz = encode_ref(body, contact)
    assert n.min() > 0.1 and gz.min() >= -0.9, f'{what}: ill-conditioned input (across {float(n.min()):.3f}, forward z {float(gz.min()):.3f})'
    if wide:
        assert gz.min() < 0 < gz.max(), f'{what}: the heading does not pass pi / 2'
    oc = contact.astype(np.float64).copy()
    oc[T - 1] = 0.0
    oimg, opiv = MO.get_local_markers_4chan(body.astype(np.float64), oc)
    S_all = np.abs(ref).max()
    assert np.abs(oimg.astype(LD) - ref).max() <= 1e-9 * S_all and abs(float(opiv[0]) - float(piv)) <= 1e-9, f'{what}: restatement vs oracle'
    d, Tm = 3 * M1 + 4, T - 1
    bd, cd = _t(body, dev), _t(contact, dev)
    iwhole, img = guarded(4 * Tm * d, dev)
    pwhole, pv = guarded_pivot(dev)
    rc = lib.local_markers_4chan(ptr(bd), ptr(cd), T, M1, ptr(img), ptr(pv), lib.stream(dev))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    got = guards_intact(iwhole, 4 * Tm * d, what).numpy().reshape(4, Tm, d)
    pgot = pivot_result(pwhole, what)
    assert np.isfinite(pgot), f'{what}: rot_0_pivot not written'
    for ch in range(4):
        marker_bound('markers encode', got[ch], ref[ch], f'{what} channel {ch}')
    assert np.array_equal(_bits32(got[0, :, 3 * M1:]), _bits32(contact[:Tm])), f'{what}: contact columns are not a copy'
    for ch in (1, 2, 3):
        assert (_bits32(got[ch]) == _bits32(got[ch])[:, :1]).all(), f'{what}: channel {ch} is not one value repeated over d'
    perr = abs(LD(pgot) - piv)
    record('markers rot_0_pivot', float(perr / 2.0 ** -48), float(perr))
    assert perr <= 2.0 ** -48, f'{what}: rot_0_pivot {float(perr):.3e} from the reference'


def check_encode_refusals(lib, dev):
    body = torch.randn(257, 68, 3).to(dev)
    contact = torch.ones(257, 4).to(dev)
    s = lib.stream(dev)
    for T, M1 in ((1, 68), (257, 68), (10, 58)):
        iwhole, img = guarded(4 * 256 * (3 * 68 + 4), dev)
        pwhole, pv = guarded_pivot(dev)
        rc = lib.local_markers_4chan(ptr(body), ptr(contact), T, M1, ptr(img), ptr(pv), s)
        _sync(lib)
        assert rc == ERR_SHAPE, (T, M1, rc)
        assert torch.isnan(iwhole.cpu()).all() and torch.isnan(pwhole.cpu()).all(), f'refused local_markers_4chan (T {T} M1 {M1}) wrote'
    for k in range(4):
        a = [ptr(body), ptr(contact), ptr(img), ptr(pv)]
        a[k] = None
        assert lib.local_markers_4chan(a[0], a[1], 10, 68, a[2], a[3], s) == ERR_ARG, k
    _sync(lib)
    assert torch.isnan(iwhole.cpu()).all() and torch.isnan(pwhole.cpu()).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 1b. lemo_reconstruct_global_body / _dev

DEC_T = (1, 2, 65, 255, 256)
REC_J = (1, 5, 68)
DECODE_J = (2, 68)


def rot_y(th, x, z):
    c, s = np.cos(th), np.sin(th)
    return c * x + s * z, -s * x + c * z


def integrate(r, x, z, rot0):
    """heading before every frame and translation before every frame from the increments (all long double)"""
    ang = -np.cumsum(r)
    dx, dz = rot_y(ang - rot0, x, z)
    tx, tz = np.cumsum(dx), np.cumsum(dz)
    zero = np.zeros(1, LD)
    return np.concatenate([zero, ang[:-1]]) - rot0, np.concatenate([zero, tx[:-1]]), np.concatenate([zero, tz[:-1]])


def reconstruct_ref(inp, rot0):
    b = inp.astype(LD)
    th, ox, oz = integrate(b[:, -1, 2], b[:, -1, 0], b[:, -1, 1], LD(rot0))
    p = b[:, 1:-1]
    rx, rz = rot_y(th[:, None], p[..., 0], p[..., 1])
    return np.stack([rx + ox[:, None], rz + oz[:, None], p[..., 2]], -1)


def reconstruct_inputs(T, J, seed):
    rng = np.random.default_rng(seed)
    inp = rng.normal(0, 0.5, (T, J + 2, 3))
    inp[:, -1] = np.stack([rng.normal(0.004, 0.02, T), rng.normal(0.012, 0.02, T), rng.normal(0.002, 0.03, T)], -1)
    inp[:, 0] = NAN                                                      # the reference slot is dropped unread
    return inp.astype(np.float32), float(rng.uniform(-1.5, 1.5))


def check_reconstruct(lib, dev, T, J):
    what = f'reconstruct_global_body T {T} J {J}'
    inp, rot0 = reconstruct_inputs(T, J, seed=77 * T + J)
    ref = reconstruct_ref(inp, rot0)
    o_in = inp.astype(np.float64).copy()
    o_in[:, 0] = 0.0
    orc = MO.reconstruct_global_body(o_in, np.array([rot0]))
    S = np.abs(ref).max()
    assert np.abs(orc.astype(LD) - ref).max() <= 1e-9 * S, f'{what}: restatement vs oracle'
    ind = _t(inp, dev)
    pv = torch.tensor([rot0], dtype=torch.float64).to(dev)
    s = lib.stream(dev)
    outs = []
    for form in ('host', 'dev', 'dev'):
        whole, out = guarded(T * J * 3, dev)
        rc = (lib.reconstruct_global_body(ptr(ind), T, J, rot0, ptr(out), s) if form == 'host' else
              lib.reconstruct_global_body_dev(ptr(ind), T, J, ptr(pv), ptr(out), s))
        _sync(lib)
        assert rc == 0, f'{what}: refused ({rc})'
        outs.append(guards_intact(whole, T * J * 3, what).clone())
    same_bits(outs[0], outs[1], f'{what}: _dev differs from the host pivot')
    same_bits(outs[1], outs[2], f'{what}: two launches differ')
    got = outs[0].numpy().reshape(T, J, 3)
    marker_bound('markers reconstruct', got, ref, what)
    assert np.array_equal(_bits32(got[..., 2]), _bits32(inp[:, 1:-1, 2])), f'{what}: the third coordinate is not its input'


def check_reconstruct_refusals(lib, dev):
    ind = torch.randn(257, 7, 3).to(dev)
    pv = torch.zeros(1, dtype=torch.float64).to(dev)
    s = lib.stream(dev)
    whole, out = guarded(257 * 5 * 3, dev)
    for T, J in ((0, 5), (257, 5), (10, 0)):
        assert lib.reconstruct_global_body(ptr(ind), T, J, 0.3, ptr(out), s) == ERR_SHAPE, (T, J)
        assert lib.reconstruct_global_body_dev(ptr(ind), T, J, ptr(pv), ptr(out), s) == ERR_SHAPE, (T, J)
    assert lib.reconstruct_global_body(None, 10, 5, 0.3, ptr(out), s) == ERR_ARG
    assert lib.reconstruct_global_body(ptr(ind), 10, 5, 0.3, None, s) == ERR_ARG
    assert lib.reconstruct_global_body_dev(None, 10, 5, ptr(pv), ptr(out), s) == ERR_ARG
    assert lib.reconstruct_global_body_dev(ptr(ind), 10, 5, None, ptr(out), s) == ERR_ARG
    assert lib.reconstruct_global_body_dev(ptr(ind), 10, 5, ptr(pv), None, s) == ERR_ARG
    _sync(lib)
    assert torch.isnan(whole.cpu()).all(), 'a refused reconstruct_global_body wrote its output'


# ---------------------------------------------------------------------------------------------------------------------------
# 1c. lemo_decode_clip

PLANTED = (0.0, 1e-3, -1e-3, 80.0, -80.0, float('inf'), float('-inf'))
POST_SHIFT = 0.37


def post_transform():
    """(z shift, M [3, 3], t [3]) float32: a rotation about (1, 2, 3) by 0.7 rad (no zero entry, not symmetric), |t| = 2"""
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * Kx @ Kx
    t = 2.0 * np.array([2.0, -1.0, 2.0]) / 3.0
    return np.float32(POST_SHIFT), M.astype(np.float32), t.astype(np.float32)


def decode_inputs(T, J, seed):
    """rec [d, T], traj [3, T] float32, stats [2 d + 4] float64, rot0: NaN in every entry the kernel does not read"""
    rng = np.random.default_rng(seed)
    d = 3 * J + 4
    rec = rng.normal(0, 1.0, (d, T))
    rec[:3] = NAN                                                        # the pelvis rows are dropped unread
    x = rng.normal(0, 2.0, (4, T))
    x = np.where(np.abs(x) < 1e-3, 1e-3, x)                              # logits with |x| >= 1e-3 ...
    flat = x.reshape(-1)
    pos = rng.permutation(4 * T)[:len(PLANTED)]
    flat[pos] = PLANTED[:len(pos)]                                       # ... and the planted ones
    rec[d - 4:] = flat.reshape(4, T)
    traj = rng.normal(0, 1.0, (3, T))
    stats = np.full(2 * d + 4, NAN)
    stats[3:d - 4] = rng.normal(0, 0.4, d - 7)                           # mean of the marker rows
    stats[d + 3:2 * d - 4] = rng.uniform(0.05, 0.3, d - 7)               # std
    stats[2 * d:] = [0.008, 0.02, 0.001, 0.03]
    return rec.astype(np.float32), traj.astype(np.float32), stats, float(rng.uniform(-1.5, 1.5))


def decode_ref(rec, traj, stats, rot0, J):
    """(labels [T, 4], markers [T, J - 1, 3] long double, float32 third coordinate) with the documented float32 stores"""
    d, T = rec.shape
    mean, sd = stats[:d], stats[d:2 * d]
    mxy, sxy, mr, sr = stats[2 * d:]
    f64 = lambda a: a.astype(np.float64)
    vx = (f64(traj[0]) * sxy + mxy).astype(np.float32)
    vz = (f64(traj[1]) * sxy + mxy).astype(np.float32)
    r = (f64(traj[2]) * sr + mr).astype(np.float32)
    th, ox, oz = integrate(r.astype(LD), vx.astype(LD), vz.astype(LD), LD(rot0))
    p = (f64(rec[3:d - 4]) * sd[3:d - 4, None] + mean[3:d - 4, None]).astype(np.float32)      # [3 (J - 1), T]
    p = p.reshape(J - 1, 3, T).transpose(2, 0, 1)                                            # [T, J - 1, 3]
    rx, rz = rot_y(th[:, None], p[..., 0].astype(LD), p[..., 1].astype(LD))
    ref = np.stack([rx + ox[:, None], rz + oz[:, None], p[..., 2].astype(LD)], -1)
    lbl = (rec[d - 4:].T > 0).astype(np.float32)
    return lbl, ref, p[..., 2]


def check_decode(lib, dev, T, J):
    what = f'decode_clip T {T} J {J}'
    rec, traj, stats, rot0 = decode_inputs(T, J, seed=31 * T + J)
    lbl_ref, ref, third = decode_ref(rec, traj, stats, rot0, J)
    logits = rec[3 * J:].reshape(-1)
    assert ((np.abs(logits) >= 1e-3) | (logits == 0)).all() and (logits == 0).sum() == 1
    Jm = J - 1
    rd, td, sd_, pv = _t(rec, dev), _t(traj, dev), _t(stats, dev, np.float64), torch.tensor([rot0], dtype=torch.float64).to(dev)
    shift, M, t = post_transform()
    post = _t(np.concatenate([[shift], M.reshape(-1), t]), dev)
    s = lib.stream(dev)
    res = {}
    for name, pp in (('null', None), ('null2', None), ('post', post)):
        lwhole, lbl = guarded(T * 4, dev)
        mwhole, mk = guarded(T * Jm * 3, dev)
        rc = lib.decode_clip(ptr(rd), ptr(td), ptr(sd_), ptr(pv), ptr(pp), T, J, ptr(lbl), ptr(mk), s)
        _sync(lib)
        assert rc == 0, f'{what}: refused ({rc})'
        res[name] = (guards_intact(lwhole, T * 4, what + ' labels').clone(), guards_intact(mwhole, T * Jm * 3, what + ' markers').clone())
    for k in (0, 1):
        same_bits(res['null'][k], res['null2'][k], f'{what}: two launches differ')
    same_bits(res['null'][0], res['post'][0], f'{what}: post changes the labels')
    assert np.array_equal(res['null'][0].numpy().reshape(T, 4), lbl_ref), f'{what}: labels are not (x > 0)'
    got = res['null'][1].numpy().reshape(T, Jm, 3)
    S = np.abs(ref).max()
    marker_bound('markers decode', got, ref, what, S)
    assert np.array_equal(_bits32(got[..., 2]), _bits32(third)), f'{what}: the third coordinate is not the de-normalised float32'
    # post: the float32 affine map of the kernel's own post == NULL output, in float64
    g = got.astype(np.float64)
    g[..., 2] = (got[..., 2] + shift).astype(np.float64)                 # one float32 addition, as the kernel performs it
    Md, tdd = M.astype(np.float64), t.astype(np.float64)
    pref = g @ Md + tdd
    terms = np.abs(g) @ np.abs(Md) + np.abs(tdd)
    prop = (U * np.abs(np.asarray(ref, np.float64)) + 2.0 ** -40 * float(S)) @ np.abs(Md)
    gp = res['post'][1].numpy().reshape(T, Jm, 3)
    assert np.isfinite(gp).all(), f'{what} post: unwritten outputs'
    ratio = float((np.abs(gp.astype(np.float64) - pref) / (4 * U * terms + prop)).max())
    record('markers decode post', ratio, float(np.abs(gp.astype(np.float64) - pref).max()))
    print(f'{what} post: worst error / bound = {ratio:.4f}')
    assert ratio <= 1.0, f'{what} post: {ratio:.3f} x (4 u sum |terms| + propagated)'


def check_decode_refusals(lib, dev):
    J = 3
    d = 3 * J + 4
    rec, traj = torch.randn(d, 257).to(dev), torch.randn(3, 257).to(dev)
    stats, pv = torch.ones(2 * d + 4, dtype=torch.float64).to(dev), torch.zeros(1, dtype=torch.float64).to(dev)
    s = lib.stream(dev)
    lwhole, lbl = guarded(257 * 4, dev)
    mwhole, mk = guarded(257 * J * 3, dev)
    assert lib.decode_clip(ptr(rec), ptr(traj), ptr(stats), ptr(pv), None, 10, 1, ptr(lbl), ptr(mk), s) == ERR_SHAPE
    assert lib.decode_clip(ptr(rec), ptr(traj), ptr(stats), ptr(pv), None, 257, J, ptr(lbl), ptr(mk), s) == ERR_SHAPE
    for k in range(6):
        a = [ptr(rec), ptr(traj), ptr(stats), ptr(pv), ptr(lbl), ptr(mk)]
        a[k] = None
        assert lib.decode_clip(a[0], a[1], a[2], a[3], None, 10, J, a[4], a[5], s) == ERR_ARG, k
    _sync(lib)
    assert torch.isnan(lwhole.cpu()).all() and torch.isnan(mwhole.cpu()).all(), 'a refused decode_clip wrote'


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lemo_smooth_loss

SMOOTH_SHAPES = (                 # (H, W, C)
    (1, 1, 8),                    # no pair: dpre exactly 0, sum exactly 0
    (1, 2, 8),
    (3, 5, 8),                    # less than one block
    (8, 8, 64),                   # exactly 1024 items
    (1, 65, 64),                  # one item pair into the second block
    (5, 13, 32),
    (9, 21, 64),
    (2, 257, 8),
)
SMOOTH_W = 0.5


def smooth_ref(z, W, coef2):
    """float64 (dpre, elementwise bound / u, sum of squares) with the kernel's float32 slope"""
    z = z.double()
    c, l, r = z, F.pad(z, (1, 0))[..., :-1], F.pad(z, (0, 1))[..., 1:]
    hasl, hasr = torch.arange(W) >= 1, torch.arange(W) <= W - 2
    dl, dr = torch.where(hasl, c - l, 0.0), torch.where(hasr, r - c, 0.0)
    g = torch.where(z > 0, 1.0, SLOPE32).double()
    return coef2 * (dl - dr) * g, 4 * abs(coef2) * g * (dl.abs() + dr.abs()), float((dr ** 2).sum())


def check_smooth(lib, dev, H, W, Cn):
    what = f'smooth_loss {H} x {W} C {Cn}'
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + Cn)
    z = F.leaky_relu(torch.randn(Cn, H, W, generator=gen), 0.2)
    coef2 = float(np.float32(SMOOTH_W * 2.0 / (Cn * H * max(W - 1, 1))))
    ref, tol, sq64 = smooth_ref(z, W, coef2)
    d10 = stencil64(z.double(), W, coef2)[0]                             # the statement the turn test uses (slope 0.2 in float64)
    assert ((ref - d10).abs() <= 2.0 ** -25 * d10.abs()).all(), f'{what}: the two float64 statements disagree'
    nb = lib.smooth_loss_blocks(H, W, Cn)
    assert nb == (2 * H * W * (Cn // 8) + 1023) // 1024, f'{what}: {nb} blocks'
    G, Hp, Wp = Cn // 8, H + 2, W + 2
    n = G * Hp * Wp * 8
    zwhole, zb = sentinel_cg8p(Cn, H, W, dev)                            # NaN border, NaN behind
    zb.view(G, Hp, Wp, 8)[:, 1:-1, 1:-1, :] = z.reshape(G, 8, H, W).permute(0, 2, 3, 1).to(dev)
    inner = torch.zeros(Hp, Wp, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    s = lib.stream(dev)
    outs = []
    for _ in range(2):
        dwhole, dp = guarded(n, dev)
        pwhole, part = guarded(nb + 16, dev)
        rc = lib.smooth_loss(ptr(zb), ptr(dp), ptr(part), H, W, Cn, coef2, s)
        _sync(lib)
        assert rc == 0, f'{what}: refused ({rc})'
        d = guards_intact(dwhole, n, what + ' dpre').view(G, Hp, Wp, 8)
        assert torch.isnan(d[:, ~inner]).all(), f'{what}: wrote into the border of dpre'
        p = guards_intact(pwhole, nb + 16, what + ' partial')
        assert torch.isnan(p[nb:]).all(), f'{what}: wrote past lemo_smooth_loss_blocks() partials'
        assert torch.isfinite(d[:, inner]).all() and torch.isfinite(p[:nb]).all(), f'{what}: unwritten or non-finite outputs'
        outs.append((d[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).reshape(Cn, H, W).clone(), p[:nb].clone()))
    same_bits(outs[0][0], outs[1][0], f'{what}: two launches differ (dpre)')
    same_bits(outs[0][1], outs[1][1], f'{what}: two launches differ (partial)')
    got, part = outs[0]
    err = (got.double() - ref).abs()
    bound = U * tol
    if W == 1:
        assert (got == 0).all() and float(part.double().sum()) == 0.0, f'{what}: no pair, yet a nonzero output'
    assert (err[bound == 0] == 0).all(), f'{what}: nonzero error where the bound is zero'
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    record('smooth_loss dpre', ratio, float(err.max()))
    ssum = float(part.double().sum())
    rs = abs(ssum - sq64) / (32 * U * sq64) if sq64 > 0 else 0.0
    record('smooth_loss sum', rs, abs(ssum - sq64) / sq64 if sq64 > 0 else 0.0)
    print(f'{what}: dpre error / bound {ratio:.3f}, sum error / bound {rs:.3f}')
    assert ratio <= 1.0, f'{what}: dpre {ratio:.3f} x its bound'
    assert abs(ssum - sq64) <= 32 * U * sq64, f'{what}: sum of squares {ssum!r} vs float64 {sq64!r}'


def check_smooth_refusals(lib, dev):
    H, W, Cn = 3, 5, 16
    zwhole, zb = sentinel_cg8p(Cn, H, W, dev)
    zb.fill_(0.5)
    n = 2 * 5 * 7 * 8
    dwhole, dp = guarded(n, dev)
    pwhole, part = guarded(8, dev)
    s = lib.stream(dev)
    for h, w, c in ((H, W, 12), (0, W, Cn), (H, 0, Cn), (H, W, 0), (-1, W, Cn), (H, W, 4)):
        assert lib.smooth_loss(ptr(zb), ptr(dp), ptr(part), h, w, c, 0.1, s) == ERR_SHAPE, (h, w, c)
    assert lib.smooth_loss(None, ptr(dp), ptr(part), H, W, Cn, 0.1, s) == ERR_ARG
    assert lib.smooth_loss(ptr(zb), None, ptr(part), H, W, Cn, 0.1, s) == ERR_ARG
    _sync(lib)
    assert torch.isnan(dwhole.cpu()).all() and torch.isnan(pwhole.cpu()).all(), 'a refused smooth_loss wrote'


# ---------------------------------------------------------------------------------------------------------------------------
# 3. lemo_adam_flat / lemo_adam_flat_ctr

ADAM_T = (1, 2, 3, 7, 1000, 20000, 10 ** 6)
ADAM_N = (1, 255, 256, 257, 4099)
ADAM_LR = (0.01, 0.005, 0.1, 0.003, 3e-6, float(np.float32(1 / 3)))      # the last is no short decimal: lr_decimal passes it through


def adam_state(n, t, seed):
    g_ = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) * torch.rand(n, generator=g_)
    if t == 1:
        return p0, g, torch.zeros(n), torch.zeros(n)
    m0 = torch.randn(n, generator=g_) * 0.3
    v0 = (torch.randn(n, generator=g_) * 0.3) ** 2 + 1e-6
    assert (m0 != 0).all() and (v0 > 0).all()
    return p0, g, m0, v0


def torch_adam(p0, g, m0, v0, t, lr):
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, foreach=False)
    opt.state[pt] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m0.clone(), 'exp_avg_sq': v0.clone()}
    pt.grad = g.clone()
    opt.step()
    st = opt.state[pt]
    assert float(st['step']) == t
    return pt.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()


def run_adam(lib, dev, p0, g, m0, v0, lr, step=None, ctr=None, what='adam_flat'):
    """one lemo_adam_flat (or _ctr) call on guarded buffers -> (p, m, v) on the CPU"""
    n = p0.numel()
    bufs = []
    for src in (p0, m0, v0):
        whole, view = guarded(n, dev)
        view.copy_(src)
        bufs.append((whole, view))
    gd = g.to(dev)
    (pw, p), (mw, m), (vw, v) = bufs
    rc = (lib.adam_flat(ptr(p), ptr(gd), ptr(m), ptr(v), n, lr, step, lib.stream(dev)) if ctr is None else
          lib.adam_flat_ctr(ptr(p), ptr(gd), ptr(m), ptr(v), n, lr, ptr(ctr), lib.stream(dev)))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    return tuple(guards_intact(w_, n, what).clone() for w_ in (pw, mw, vw))


def adam_ops32(p0, m, v, t, lr):
    """the parameter update of common.hpp operation for operation in numpy float32 (every operation one IEEE rounding), the two
    coefficients from the host's double pow: what the kernel gives when the device pow returns the same doubles"""
    f = np.float32
    neg_step, bc2s = f(-(lr / (1.0 - 0.9 ** t))), f(np.sqrt(1.0 - 0.999 ** t))
    out = p0.numpy() + (neg_step * m.numpy()) / (np.sqrt(v.numpy()) / bc2s + f(1e-8))
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def _share(key, share):
    r, e, k = RATIOS.get(key, (0.0, 1.0, 0))
    RATIOS[key] = (max(r, 1.0 - share), min(e, share), k + 1)
    FAMILIES.add(key)


def check_adam(lib, dev, t, lr):
    share, ops, cnt = 0.0, 0.0, 0
    for n in ADAM_N:
        what = f'adam_flat t {t} n {n} lr {lr:g}'
        p0, g, m0, v0 = adam_state(n, t, seed=n + 13 * (t % 9973))
        pt, mt, vt = torch_adam(p0, g, m0, v0, t, lr)
        p, m, v = run_adam(lib, dev, p0, g, m0, v0, lr, step=t, what=what)
        same_bits(m, mt, f'{what}: exp_avg differs from torch')
        same_bits(v, vt, f'{what}: exp_avg_sq differs from torch')
        delta = -(lr / (1.0 - 0.9 ** t)) * m.double() / (v.double().sqrt() / np.sqrt(1.0 - 0.999 ** t) + 1e-8)
        bound = 2 * U * torch.maximum(p0.abs(), pt.abs()).double() + 6 * U * delta.abs()
        err = (p.double() - pt.double()).abs()
        ratio = float((err / bound).max())
        share += float((p.view(torch.int32) == pt.view(torch.int32)).sum())
        ops += float((p.view(torch.int32) == adam_ops32(p0, m, v, t, lr).view(torch.int32)).sum())
        cnt += n
        record('adam parameter', ratio, float(err.max()))
        assert ratio <= 1.0, f'{what}: parameter {ratio:.3f} x (2 u max |p| + 6 u |delta|) from torch'
    _share(SHARE, share / cnt)
    _share(SHARE_OPS, ops / cnt)
    print(f'adam_flat t {t} lr {lr:g}: {share / cnt:.4f} of the parameters bit-equal with torch, {ops / cnt:.4f} with the float32 restatement')


def check_adam_ctr(lib, dev, t, lr=0.003, n=257):
    what = f'adam_flat_ctr t {t}'
    p0, g, m0, v0 = adam_state(n, t + 1, seed=5 + t)
    cwhole, ctr = guarded(1, dev, dtype=torch.int32, fill=t)
    st_c, st_f = (p0, m0, v0), (p0, m0, v0)
    for k in (1, 2):
        st_c = run_adam(lib, dev, st_c[0], g, st_c[1], st_c[2], lr, ctr=ctr, what=what)
        assert int(guards_intact(cwhole, 1, what + ' counter')[0]) == t + k, f'{what}: the counter did not advance by one'
        st_f = run_adam(lib, dev, st_f[0], g, st_f[1], st_f[2], lr, step=t + k, what=what)
        for a, b, name in zip(st_c, st_f, 'pmv'):
            same_bits(a, b, f'{what}: call {k} differs from adam_flat at step {t + k} ({name})')


def check_adam_refusals(lib, dev):
    n = 16
    bufs = [guarded(n, dev) for _ in range(3)]
    g = torch.randn(n).to(dev)
    (pw, p), (mw, m), (vw, v) = bufs
    cwhole, ctr = guarded(1, dev, dtype=torch.int32, fill=3)
    s = lib.stream(dev)
    assert lib.adam_flat(ptr(p), ptr(g), ptr(m), ptr(v), 0, 0.01, 1, s) == ERR_ARG
    assert lib.adam_flat(ptr(p), ptr(g), ptr(m), ptr(v), n, 0.01, 0, s) == ERR_ARG
    assert lib.adam_flat_ctr(ptr(p), ptr(g), ptr(m), ptr(v), 0, 0.01, ptr(ctr), s) == ERR_ARG
    assert lib.adam_flat_ctr(ptr(p), ptr(g), ptr(m), ptr(v), n, 0.01, None, s) == ERR_ARG
    for k in range(4):
        a = [ptr(p), ptr(g), ptr(m), ptr(v)]
        a[k] = None
        assert lib.adam_flat(a[0], a[1], a[2], a[3], n, 0.01, 1, s) == ERR_ARG, k
    _sync(lib)
    assert all(torch.isnan(w_.cpu()).all() for w_ in (pw, mw, vw)), 'a refused adam_flat wrote'
    assert int(guards_intact(cwhole, 1, 'adam_flat_ctr counter')[0]) == 3, 'a refused adam_flat_ctr advanced the counter'


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lemo_dec_end_fwd

DEC_END_SHAPES = (                # (bs, H, W, floats between two images of u beyond one image)
    (1, 1, 1, 0),                 # H W = 1
    (1, 16, 16, 0),               # 256 pixels: exactly one block
    (1, 1, 257, 0),               # one pixel past the block edge
    (3, 5, 7, 40),                # u_stride 40 floats beyond one image, the gap filled with NaN
    (2, 9, 21, 0),
)


def check_dec_end(lib, dev, bs, H, W, gap):
    what = f'dec_end_fwd bs {bs} {H} x {W}' + (f' gap {gap}' if gap else '')
    gen = torch.Generator().manual_seed(bs * 10000 + H * 100 + W)
    x = torch.randn(bs, 32, H, W, generator=gen)
    x = torch.where(x > 0, x, 0.2 * x) * 0.3
    w8, b8 = torch.randn(32, 9, generator=gen) * 0.1, torch.randn(1, generator=gen) * 0.1
    w9, b9 = torch.randn(9, generator=gen) * 0.3, torch.randn(1, generator=gen) * 0.1
    Hp, Wp = H + 2, W + 2
    img = 4 * Hp * Wp * 8
    stride = img + gap
    uw, ub = guarded(bs * stride, dev)                                   # NaN: the gaps (and the guards)
    for b in range(bs):
        v = ub[b * stride:b * stride + img].view(4, Hp, Wp, 8)
        v.zero_()                                                        # the border of u is real zero padding: it is read
        v[:, 1:-1, 1:-1, :] = x[b].reshape(4, 8, H, W).permute(0, 2, 3, 1).to(dev)
    w8d, b8d, w9d, b9d = w8.to(dev), b8.to(dev), w9.to(dev), b9.to(dev)
    inner = torch.zeros(Hp, Wp, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    s = lib.stream(dev)
    outs = []
    for _ in range(2):
        pair = []
        for _k in range(2):
            whole, view = guarded(bs * Hp * Wp, dev, fill=0.0)
            view.view(bs, Hp, Wp)[:, 1:-1, 1:-1] = NAN
            pair.append((whole, view))
        rc = lib.dec_end_fwd(ptr(ub), stride, ptr(w8d), ptr(b8d), ptr(w9d), ptr(b9d), ptr(pair[0][1]), ptr(pair[1][1]), bs, H, W, s)
        _sync(lib)
        assert rc == 0, f'{what}: refused ({rc})'
        res = []
        for (whole, _v), name in zip(pair, ('r1', 'rec')):
            o = guards_intact(whole, bs * Hp * Wp, f'{what} {name}').view(bs, Hp, Wp)
            assert (o[:, ~inner].view(torch.int32) == 0).all(), f'{what}: wrote into the zero border of {name}'
            assert torch.isfinite(o[:, inner]).all(), f'{what}: unwritten or non-finite {name}'
            res.append(o[:, 1:-1, 1:-1].clone())
        outs.append(res)
    guards_intact(uw, bs * stride, what + ' u')
    for k, name in ((0, 'r1'), (1, 'rec')):
        same_bits(outs[0][k], outs[1][k], f'{what}: two launches differ ({name})')
    r1, rec = outs[0]
    xd = x.double()
    W8, W9 = w8.double().view(32, 1, 3, 3), w9.double().view(1, 1, 3, 3)
    ref1 = F.leaky_relu(F.conv_transpose2d(xd, W8, b8.double(), padding=1), 0.2)[:, 0]
    mag1 = (F.conv_transpose2d(xd.abs(), W8.abs(), padding=1) + b8.double().abs())[:, 0]
    ra, _ = check_close(r1, ref1, mag1, 'fp32', what + ' (r1)')
    r1d = r1.double()[:, None]
    ref2 = (F.conv_transpose2d(r1d, W9, padding=1) + b9.double())[:, 0]
    mag2 = (F.conv_transpose2d(r1d.abs(), W9.abs(), padding=1) + b9.double().abs())[:, 0]
    rb, _ = check_close(rec, ref2, mag2, 'fp32', what + ' (rec)')
    record('dec_end r1', ra / TAU['fp32'], ra)
    record('dec_end rec', rb / TAU['fp32'], rb)
    print(f'{what}: r1 {ra:.3e} x mag, rec {rb:.3e} x mag (tau {TAU["fp32"]:.1e})')


def check_dec_end_refusals(lib, dev):
    bs, H, W = 2, 3, 4
    img = 4 * 5 * 6 * 8
    u = torch.zeros(bs * img).to(dev)
    w8, b8, w9, b9 = torch.randn(32, 9).to(dev), torch.randn(1).to(dev), torch.randn(9).to(dev), torch.randn(1).to(dev)
    rw, r1 = guarded(bs * 30, dev)
    cw, rec = guarded(bs * 30, dev)
    s = lib.stream(dev)
    full = [ptr(u), ptr(w8), ptr(b8), ptr(w9), ptr(b9), ptr(r1), ptr(rec)]
    assert lib.dec_end_fwd(full[0], img, *full[1:], 0, H, W, s) == ERR_ARG
    assert lib.dec_end_fwd(full[0], -1, *full[1:], bs, H, W, s) == ERR_ARG
    for k in range(7):
        a = list(full)
        a[k] = None
        assert lib.dec_end_fwd(a[0], img, *a[1:], bs, H, W, s) == ERR_ARG, k
    _sync(lib)
    assert torch.isnan(rw.cpu()).all() and torch.isnan(cw.cpu()).all(), 'a refused dec_end_fwd wrote'
