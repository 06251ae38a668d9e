"""Shape sweep of the hand-written 3x3 convolution kernels against float64 (tests/test_gpu_conv_shapes.py on the MI355X,
tests/test_conv_shapes_emu.py on the host-emulated build of the same sources).

Every case launches one kernel through the C ABI on the current stream and checks four things:
  1. elementwise error: |got - ref| <= tau * mag at every output element, where mag = |x| (*) |w| + |b| is the same operator
     applied in float64 to the absolute values (times lrelu'(aux) for backward-data), and tau is set per arithmetic; plus a
     max |err| / max |ref| gate no looser than the existing single-shape tests';
  2. write set: the padded border of the output and a guard region allocated past its end hold a NaN sentinel before the
     launch, and still hold it after (the same for documented scratch sizes);
  3. determinism: a second launch on the same inputs gives identical bits;
  4. refusal: where the *_supported predicate says no, the launch returns LEMO_ERR_SHAPE and writes nothing.
The float64 references run on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from lemo_amd._hip import ptr
from lemo_amd.assets import load_assets
from lemo_amd.priors import (enc_layer_keys, pack_conv3x3, pack_conv3x3_bwd, pack_conv3x3_gmajor, pack_conv3x3_bwd_gmajor,
                             pack_conv3x3_split, pack_conv3x3_bwd_split, pack_conv3x3_split_f16, pack_conv3x3_bwd_split_f16,
                             pack_conv3x3_wino_f16, pack_conv3x3_bwd_wino_f16, to_cg8p, from_cg8p)

ERR_SHAPE = 10001
ERR_ARG = 10002
SLOPE = 0.2
GUARD = 4096                     # sentinel floats allocated past the end of every output / documented scratch size

# tau per arithmetic: |got - ref| <= tau * (|x| (*) |w| + |b|) elementwise, 3 x the worst ratio the MI355X gave over the whole sweep
# of tests/test_gpu_conv_shapes.py: fp32 FMA / MFMA 5.37e-7 (conv3x3_mfma_lds; wgrad3x3_batched 7.3e-8), split-bf16 2.42e-7,
# split-f16 2.25e-7 (pair_f16; the single-layer kernel 1.77e-7), Winograd-f16 1.46e-7, ae_conv_f16 (scales from tensor maxima) 2.01e-7;
# ae_conv (fp32) 3.41e-7.  The emulator's ratios are below these.
TAU = {'fp32': 1.6e-6, 'split_bf16': 7.2e-7, 'split_f16': 6.7e-7, 'wino_f16': 4.3e-7, 'ae_f16': 6.0e-7}
# max |err| / max |ref| (the existing gates: 2e-6 for the split kernels at 245 x 134, 1e-6 for ae_conv_f16 at 7 x 9)
REL = {'fp32': 2e-6, 'split_bf16': 2e-6, 'split_f16': 2e-6, 'wino_f16': 2e-6, 'ae_f16': 1e-6}

_ENC = None


def enc_weight(cin, cout):
    """(w [cout][cin][3][3], b [cout]) float32: a real encoder layer of that channel shape (runs/15217) where one exists, else seeded
    random weights of the same magnitude"""
    global _ENC
    if _ENC is None:
        _ENC = load_assets()['enc_w']
    for k in enc_layer_keys():
        w = np.asarray(_ENC[k + '.weight'], np.float32)
        if w.shape[0] == cout and w.shape[1] == cin:
            return torch.from_numpy(w.copy()), torch.from_numpy(np.asarray(_ENC[k + '.bias'], np.float32).copy())
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    return torch.randn(cout, cin, 3, 3, generator=g) * 0.06, torch.randn(cout, generator=g) * 0.1


class Rec:
    """worst measured error ratio per arithmetic (printed by the GPU module: where TAU comes from)"""
    worst = {}

    @classmethod
    def add(cls, arith, ratio, rel):
        a, r = cls.worst.get(arith, (0.0, 0.0))
        cls.worst[arith] = (max(a, ratio), max(r, rel))


# ---------------------------------------------------------------------------------------------------------------------------
# buffers with sentinels

def sentinel_cg8p(C, H, W, dev):
    """(whole, view): a CG8P buffer [C/8][(H+2)(W+2)][8] filled with NaN, followed by GUARD NaN floats"""
    n = (C // 8) * (H + 2) * (W + 2) * 8
    whole = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=dev)
    return whole, whole[:n].view(C // 8, (H + 2) * (W + 2), 8)


def sentinel_flat(n, dev, fill=float('nan')):
    whole = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=dev)
    whole[:n] = fill
    return whole, whole[:n]


def check_cg8p_write_set(whole, C, H, W, what):
    """interior finite, border and guard still NaN"""
    w = whole.cpu()
    n = (C // 8) * (H + 2) * (W + 2) * 8
    assert torch.isnan(w[n:]).all(), f'{what}: wrote past the end of the output'
    b = w[:n].view(C // 8, H + 2, W + 2, 8)
    inner = torch.zeros(H + 2, W + 2, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    assert torch.isnan(b[:, ~inner]).all(), f'{what}: wrote into the padded border'
    assert torch.isfinite(b[:, inner]).all(), f'{what}: left interior pixels unwritten (or non-finite)'


def check_flat_write_set(whole, n, what, finite=True):
    w = whole.cpu()
    assert torch.isnan(w[n:]).all(), f'{what}: wrote past its documented size'
    if finite:
        assert torch.isfinite(w[:n]).all(), f'{what}: left entries unwritten (or non-finite)'


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references

def lrelu_d(aux):
    return torch.where(aux > 0, 1.0, SLOPE).double()


def ref_layer(x, w, b, epi, aux=None):
    """(ref, mag) [Cout, H, W] float64 of one layer: epi 0 lrelu(conv + b), 1 conv_transpose(x, w) * lrelu'(aux), 2 conv + b"""
    xd, wd = x[None].double(), w.double()
    if epi == 1:
        s = lrelu_d(aux)
        return (F.conv_transpose2d(xd, wd, padding=1)[0] * s, F.conv_transpose2d(xd.abs(), wd.abs(), padding=1)[0] * s)
    pre = F.conv2d(xd, wd, b.double(), padding=1)[0]
    mag = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), padding=1)[0]
    return (F.leaky_relu(pre, SLOPE) if epi == 0 else pre), mag


def check_close(got, ref, mag, arith, what):
    got = got.double()
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), what
    zero = mag == 0
    assert (err[zero] == 0).all(), f'{what}: nonzero result where every product is zero'
    ratio = float((err[~zero] / mag[~zero]).max()) if (~zero).any() else 0.0
    rel = float(err.max() / ref.abs().max().clamp_min(1e-300))
    Rec.add(arith, ratio, rel)
    Rec.add(arith + ':' + what.split()[0], ratio, rel)
    if ratio > TAU[arith]:
        i = int((err / mag.clamp_min(1e-300)).argmax())
        idx = np.unravel_index(i, tuple(ref.shape))
        raise AssertionError(f'{what}: elementwise error {ratio:.3e} x mag > tau {TAU[arith]:.1e} at {idx} '
                             f'(got {float(got.flatten()[i]):.8e}, ref {float(ref.flatten()[i]):.8e})')
    assert rel < REL[arith], f'{what}: max err / max ref {rel:.3e} >= {REL[arith]:.1e}'
    return ratio, rel


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: two launches on the same inputs differ'


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def layer_inputs(cin, cout, H, W, epi, seed, grad_scale=1e-6):
    """input [cin, H, W] (post-activation-like for the forward epilogues, gradient-sized for backward-data) and aux [cin', H, W]"""
    g = torch.Generator().manual_seed(seed)
    if epi == 1:
        return torch.randn(cin, H, W, generator=g) * grad_scale, torch.randn(cout, H, W, generator=g)
    x = torch.randn(cin, H, W, generator=g)
    return torch.where(x > 0, x, SLOPE * x) * 0.3, None


def _stream(lib, dev):
    return lib.stream(dev)


def _sync(lib):
    if not lib.is_emu:
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# single-layer kernels

SINGLE = {                        # kernel -> (arithmetic, channel pairs, epilogues)
    'mfma_v0': ('fp32', [(64, 64), (32, 64), (64, 32)], (0, 1, 2)),
    'mfma_v1': ('fp32', [(64, 64), (32, 64), (64, 32)], (0, 1, 2)),
    'mfma_lds': ('fp32', [(64, 64), (32, 64), (64, 32)], (0, 1, 2)),
    'splitk': ('fp32', [(64, 64), (64, 32)], (0, 1, 2)),
    'split_bf16': ('split_bf16', [(32, 32), (32, 64), (64, 32), (64, 64)], (0, 1, 2)),
    'split_f16': ('split_f16', [(32, 32), (32, 64), (64, 32), (64, 64)], (0, 1, 2)),
    'wino_f16': ('wino_f16', [(64, 64)], (0, 1)),
}


def supported(lib, kernel, H, W, cin, cout):
    if kernel in ('split_bf16', 'split_f16'):
        return lib.conv3x3_split_supported(H, W, cin, cout) == 1
    if kernel == 'wino_f16':
        return lib.conv3x3_wino_supported(H, W, cin, cout) == 1
    if kernel == 'mfma_lds':
        return W <= 139                          # include/lemo_hip.h: the LDS-tiled variant takes W <= 139
    return True


def run_single(lib, dev, kernel, H, W, cin, cout, epi, ks=3, refuse=False):
    """one layer of `kernel` at H x W, cin -> cout (the layer's own channel counts: backward-data maps cout -> cin of a forward
    layer cin -> cout, so the weights of the forward layer [cout][cin] are packed with the *_bwd packers and the launch is
    cout -> cin); all four checks"""
    arith = SINGLE[kernel][0]
    w, b = enc_weight(cin, cout)
    bwd = epi == 1
    kin, kout = (cout, cin) if bwd else (cin, cout)
    x, aux = layer_inputs(kin, kout, H, W, epi, seed=H * 1009 + W * 17 + cin + cout + epi)
    ref, mag = ref_layer(x, w, b, epi, aux)
    t = lambda a: (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev)
    xin = to_cg8p(x).to(dev)
    auxp = to_cg8p(aux).to(dev) if bwd else None
    bias = None if bwd else t(b)
    wt = t(pack_conv3x3_bwd(w.numpy()) if bwd else pack_conv3x3(w.numpy()))
    s = _stream(lib, dev)
    scratch = None
    if kernel in ('mfma_v0', 'mfma_v1'):
        var = int(kernel[-1])
        launch = lambda o: lib.conv3x3_mfma(ptr(xin), ptr(wt), ptr(bias), ptr(auxp), ptr(o), H, W, kin, kout, epi, var, s)
    elif kernel == 'mfma_lds':
        wt2 = t(pack_conv3x3_bwd_gmajor(w.numpy()) if bwd else pack_conv3x3_gmajor(w.numpy()))
        launch = lambda o: lib.conv3x3_mfma_lds(ptr(xin), ptr(wt), ptr(wt2), ptr(bias), ptr(auxp), ptr(o), H, W, kin, kout, epi, s)
    elif kernel == 'splitk':
        ks = min(ks, 9 * (kin // 8))                                   # the documented range: 1 <= ks <= 9 cin / 8
        n_part = ks * (kout // 8) * (H + 2) * (W + 2) * 8               # the documented scratch size
        scratch = sentinel_flat(n_part, dev, fill=0.0)
        launch = lambda o: lib.conv3x3_mfma_splitk(ptr(xin), ptr(wt), ptr(bias), ptr(auxp), ptr(o), ptr(scratch[1]), ks, H, W, kin, kout, epi, s)
    elif kernel == 'split_bf16':
        w3 = t((pack_conv3x3_bwd_split(w.numpy()) if bwd else pack_conv3x3_split(w.numpy())).view(np.int16))
        launch = lambda o: lib.conv3x3_mfma_split(ptr(xin), ptr(w3), ptr(wt), ptr(bias), ptr(auxp), ptr(o), H, W, kin, kout, epi, s)
    elif kernel == 'split_f16':
        pk, inv = pack_conv3x3_bwd_split_f16(w.numpy()) if bwd else pack_conv3x3_split_f16(w.numpy())
        w4 = t(pk.view(np.int16))
        launch = lambda o: lib.conv3x3_mfma_split_f16(ptr(xin), ptr(w4), inv, ptr(wt), ptr(bias), ptr(auxp), ptr(o), H, W, kin, kout, epi, s)
    elif kernel == 'wino_f16':
        pk, inv = pack_conv3x3_bwd_wino_f16(w.numpy()) if bwd else pack_conv3x3_wino_f16(w.numpy())
        wu = t(pk.view(np.int16))
        launch = lambda o: lib.conv3x3_wino_f16(ptr(xin), ptr(wu), inv, ptr(wt), ptr(bias), ptr(auxp), ptr(o), H, W, epi, None, s)
    else:
        raise KeyError(kernel)
    what = f'{kernel} epi {epi} {kin}->{kout} at {H} x {W}'
    whole1, o1 = sentinel_cg8p(kout, H, W, dev)
    whole2, o2 = sentinel_cg8p(kout, H, W, dev)
    if refuse:                                   # a shape listed as a refusal: the predicate must say so
        assert not supported(lib, kernel, H, W, kin, kout), f'{what}: listed as refused, but the predicate accepts it'
    if not supported(lib, kernel, H, W, kin, kout):
        rc = launch(o1)
        _sync(lib)
        assert rc == ERR_SHAPE, f'{what}: unsupported shape returned {rc}, not LEMO_ERR_SHAPE'
        assert torch.isnan(whole1.cpu()).all(), f'{what}: refused launch wrote its output'
        return None
    lib.check(launch(o1), what)
    lib.check(launch(o2), what)
    _sync(lib)
    check_cg8p_write_set(whole1, kout, H, W, what)
    if scratch is not None:
        check_flat_write_set(scratch[0], scratch[1].numel(), what + ' (split-K partial)')
    same_bits(whole1, whole2, what)
    return check_close(from_cg8p(o1.cpu(), H, W), ref, mag, arith, what)


# ---------------------------------------------------------------------------------------------------------------------------
# fused pair (variant 5)

def run_pair(lib, dev, H, W, epi):
    what = f'pair_f16 epi {epi} at {H} x {W}'
    g = torch.Generator().manual_seed(H * 7 + W + epi)
    keys = [k for k in enc_layer_keys() if np.asarray(load_assets()['enc_w'][k + '.weight']).shape[:2] == (64, 64)]
    A = load_assets()['enc_w']
    wl = [torch.from_numpy(np.asarray(A[k + '.weight'], np.float32).copy()) for k in keys[:2]]
    bl = [torch.from_numpy(np.asarray(A[k + '.bias'], np.float32).copy()) for k in keys[:2]]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = _stream(lib, dev)
    if epi == 0:
        x, _ = layer_inputs(64, 64, H, W, 0, seed=H * 7 + W)
        r1, m1 = ref_layer(x, wl[0], bl[0], 0)
        # the second layer's input is the kernel's own (fp32) intermediate: its reference is conv(mid) with mid = ref1 rounded
        (pA, iA), (pB, iB) = pack_conv3x3_split_f16(wl[0].numpy()), pack_conv3x3_split_f16(wl[1].numpy())
        args = lambda mid, out: (ptr(xin), ptr(wA), iA, ptr(bA), None, ptr(mid), ptr(wB), iB, ptr(bB), None, ptr(out), H, W, 0, None, s)
        xin, bA, bB = to_cg8p(x).to(dev), bl[0].to(dev), bl[1].to(dev)
    else:
        d2 = torch.randn(64, H, W, generator=g) * 1e-6
        a1, a0 = torch.randn(64, H, W, generator=g), torch.randn(64, H, W, generator=g)
        # backward pair (l, l-1): A = backward pack of the LATER layer (wl[1]), B of the earlier (wl[0])
        r1, m1 = ref_layer(d2, wl[1], None, 1, a1)
        (pA, iA), (pB, iB) = pack_conv3x3_bwd_split_f16(wl[1].numpy()), pack_conv3x3_bwd_split_f16(wl[0].numpy())
        xin, auxA, auxB = to_cg8p(d2).to(dev), to_cg8p(a1).to(dev), to_cg8p(a0).to(dev)
        args = lambda mid, out: (ptr(xin), ptr(wA), iA, None, ptr(auxA), None, ptr(wB), iB, None, ptr(auxB), ptr(out), H, W, 1, None, s)
    wA, wB = t(pA.view(np.int16)), t(pB.view(np.int16))
    wm1, m_1 = sentinel_cg8p(64, H, W, dev)
    wo1, o_1 = sentinel_cg8p(64, H, W, dev)
    wm2, m_2 = sentinel_cg8p(64, H, W, dev)
    wo2, o_2 = sentinel_cg8p(64, H, W, dev)
    if lib.conv3x3_pair_supported(H, W, 64, 64, 64) != 1:
        rc = lib.conv3x3_pair_f16(*args(m_1, o_1))
        _sync(lib)
        assert rc == ERR_SHAPE and torch.isnan(wo1.cpu()).all() and torch.isnan(wm1.cpu()).all(), what
        return None
    lib.check(lib.conv3x3_pair_f16(*args(m_1, o_1)), what)
    lib.check(lib.conv3x3_pair_f16(*args(m_2, o_2)), what)
    _sync(lib)
    check_cg8p_write_set(wo1, 64, H, W, what + ' (out)')
    same_bits(wo1, wo2, what)
    if epi == 0:
        check_cg8p_write_set(wm1, 64, H, W, what + ' (mid)')
        same_bits(wm1, wm2, what + ' (mid)')
        mid = from_cg8p(m_1.cpu(), H, W)
        check_close(mid, r1, m1, 'split_f16', what + ' (mid)')
        r2, m2 = ref_layer(mid, wl[1], bl[1], 0)
    else:
        assert torch.isnan(wm1.cpu()).all(), what + ': backward pair wrote `mid`'
        # reference of the second stage from the float64 intermediate; its magnitude chains both stages
        r2 = F.conv_transpose2d(r1[None], wl[0].double(), padding=1)[0] * lrelu_d(a0)
        m2 = F.conv_transpose2d(m1[None], wl[0].double().abs(), padding=1)[0] * lrelu_d(a0)
    return check_close(from_cg8p(o_1.cpu(), H, W), r2, m2, 'split_f16', what + ' (out)')


# ---------------------------------------------------------------------------------------------------------------------------
# first layer (1 channel) and the fused encoder tail

def run_c1(lib, dev, H, W):
    """conv3x3_c1 (1 -> 32, lrelu(conv + b)) and conv3x3_c1_bwd (its adjoint: 32 -> 1, no epilogue)"""
    what = f'conv3x3_c1 at {H} x {W}'
    w, b = enc_weight(1, 32)
    g = torch.Generator().manual_seed(H + 3 * W)
    x = torch.randn(1, H, W, generator=g)
    s = _stream(lib, dev)
    x0 = F.pad(x[0], (1, 1, 1, 1)).contiguous().to(dev)
    w9, bd = w.reshape(32, 9).contiguous().to(dev), b.to(dev)
    ref, mag = ref_layer(x, w, b, 0)
    (wh1, o1), (wh2, o2) = sentinel_cg8p(32, H, W, dev), sentinel_cg8p(32, H, W, dev)
    for o in (o1, o2):
        lib.check(lib.conv3x3_c1(ptr(x0), ptr(w9), ptr(bd), ptr(o), H, W, 32, s), what)
    _sync(lib)
    check_cg8p_write_set(wh1, 32, H, W, what)
    same_bits(wh1, wh2, what)
    check_close(from_cg8p(o1.cpu(), H, W), ref, mag, 'fp32', what)
    what = f'conv3x3_c1_bwd at {H} x {W}'
    dpre = torch.randn(32, H, W, generator=g) * 1e-6
    dp = to_cg8p(dpre).to(dev)
    ref = F.conv_transpose2d(dpre[None].double(), w.double(), padding=1)[0, 0]
    mag = F.conv_transpose2d(dpre[None].double().abs(), w.double().abs(), padding=1)[0, 0]
    (wd1, d1), (wd2, d2) = sentinel_flat(H * W, dev), sentinel_flat(H * W, dev)
    for d in (d1, d2):
        lib.check(lib.conv3x3_c1_bwd(ptr(dp), ptr(w9), ptr(d), H, W, 32, s), what)
    _sync(lib)
    check_flat_write_set(wd1, H * W, what)
    same_bits(wd1, wd2, what)
    return check_close(d1.cpu().view(H, W), ref, mag, 'fp32', what)


def run_enc_tail3(lib, dev, H, W):
    """d(pre-act 3) (64 ch) -> layer 2 backward-data x lrelu'(act2) -> layer 1 backward-data x lrelu'(act1) -> layer 0 adjoint -> dx0"""
    what = f'enc_tail3 at {H} x {W}'
    (w0, _), (w1, _), (w2, _) = enc_weight(1, 32), enc_weight(32, 32), enc_weight(32, 64)
    g = torch.Generator().manual_seed(5 * H + W)
    din = torch.randn(64, H, W, generator=g) * 1e-6
    act2, act1 = torch.randn(32, H, W, generator=g), torch.randn(32, H, W, generator=g)
    r2, m2 = ref_layer(din, w2, None, 1, act2)
    r1 = F.conv_transpose2d(r2[None], w1.double(), padding=1)[0] * lrelu_d(act1)
    m1 = F.conv_transpose2d(m2[None], w1.double().abs(), padding=1)[0] * lrelu_d(act1)
    ref = F.conv_transpose2d(r1[None], w0.double(), padding=1)[0, 0]
    mag = F.conv_transpose2d(m1[None], w0.double().abs(), padding=1)[0, 0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p2, i2 = pack_conv3x3_bwd_split_f16(w2.numpy())
    p1, i1 = pack_conv3x3_bwd_split_f16(w1.numpy())
    w2b, w1b, w0d = t(p2.view(np.int16)), t(p1.view(np.int16)), w0.reshape(32, 9).contiguous().to(dev)
    dinp, a2p, a1p = to_cg8p(din).to(dev), to_cg8p(act2).to(dev), to_cg8p(act1).to(dev)
    s = _stream(lib, dev)
    (wd1, d1), (wd2, d2) = sentinel_flat(H * W, dev), sentinel_flat(H * W, dev)
    for d in (d1, d2):
        lib.check(lib.enc_tail3(ptr(dinp), ptr(w2b), i2, ptr(a2p), ptr(w1b), i1, ptr(a1p), ptr(w0d), ptr(d), H, W, s), what)
    _sync(lib)
    check_flat_write_set(wd1, H * W, what)
    same_bits(wd1, wd2, what)
    return check_close(d1.cpu().view(H, W), ref, mag, 'split_f16', what)


# ---------------------------------------------------------------------------------------------------------------------------
# batched weight gradient (prior training)

def run_wgrad(lib, dev, H, W, bs, ca, cb, bias_b):
    what = f'wgrad3x3_batched {ca}x{cb} bias_b {bias_b} bs {bs} at {H} x {W}'
    g = torch.Generator().manual_seed(H * 31 + W * 7 + bs + ca + cb)
    A = torch.randn(bs, ca, H, W, generator=g)
    B = torch.randn(bs, cb, H, W, generator=g) * 1e-3
    pack = lambda T, c: (torch.stack([to_cg8p(T[i]) for i in range(bs)]) if c > 1 else F.pad(T[:, 0], (1, 1, 1, 1))).contiguous().to(dev)
    Ap, Bp = pack(A, ca), pack(B, cb)
    nws = int(lib.wgrad3x3_batched_ws_floats(H, W, bs, ca, cb))
    assert nws > 0, what
    ngb = cb if bias_b else ca
    s = _stream(lib, dev)
    outs = []
    for _ in range(2):
        ws = sentinel_flat(nws, dev)                  # scratch content on entry is not part of the contract: NaN
        gw, gb = sentinel_flat(ca * cb * 9, dev), sentinel_flat(ngb, dev)
        lib.check(lib.wgrad3x3_batched(ptr(Ap), Ap[0].numel(), ptr(Bp), Bp[0].numel(), bs, H, W, ca, cb, bias_b, ptr(ws[1]), ptr(gw[1]),
                                       ptr(gb[1]), s), what)
        outs.append((ws, gw, gb))
    _sync(lib)
    (ws, gw, gb), (_, gw2, gb2) = outs
    check_flat_write_set(ws[0], nws, what + ' (ws)', finite=False)
    check_flat_write_set(gw[0], ca * cb * 9, what + ' (gw)')
    check_flat_write_set(gb[0], ngb, what + ' (gb)')
    same_bits(gw[0], gw2[0], what + ' (gw)')
    same_bits(gb[0], gb2[0], what + ' (gb)')
    Bd, Ba = F.pad(B.double(), (1, 1, 1, 1)), F.pad(B.double().abs(), (1, 1, 1, 1))
    ref = torch.zeros(ca, cb, 3, 3, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, ky, kx] = torch.einsum('bmyx,bnyx->mn', A.double(), Bd[:, :, ky:ky + H, kx:kx + W])
            mag[:, :, ky, kx] = torch.einsum('bmyx,bnyx->mn', A.double().abs(), Ba[:, :, ky:ky + H, kx:kx + W])
    r = check_close(gw[1].cpu().view(ca, cb, 3, 3), ref, mag, 'fp32', what + ' (gw)')
    src = (B if bias_b else A).double()
    check_close(gb[1].cpu(), src.sum((0, 2, 3)), src.abs().sum((0, 2, 3)), 'fp32', what + ' (gb)')
    return r


def wgrad_refuses(lib, dev, H, W, ca, cb):
    """LEMO_ERR_SHAPE and nothing written"""
    buf = torch.zeros(1 << 16, device=dev)
    ws, gw, gb = sentinel_flat(1 << 12, dev), sentinel_flat(1 << 12, dev), sentinel_flat(64, dev)
    rc = lib.wgrad3x3_batched(ptr(buf), 0, ptr(buf), 0, 1, H, W, ca, cb, 0, ptr(ws[1]), ptr(gw[1]), ptr(gb[1]), _stream(lib, dev))
    _sync(lib)
    assert rc == ERR_SHAPE, (H, W, ca, cb, rc)
    assert all(torch.isnan(x[0].cpu()).all() for x in (ws, gw, gb))


# ---------------------------------------------------------------------------------------------------------------------------
# the encoder as the fit engine runs it (lemo_fit_forward / _backward -> csrc/enc_chain.hpp) against a float64 restatement of
# models/AE_sep.py Enc on the marker image the engine published

# max |err| / max |ref| per activation layer and of dx0, 3 x the worst the MI355X gave over the 15 engine cases (1.43e-6, 7.1e-7);
# test_gpu_parity.DX0_GATE is 7e-6
ENC_ACT_REL = 4.2e-6
ENC_DX0_REL = 2.1e-6


def _w64(A, k):
    return torch.from_numpy(np.asarray(A[k + '.weight'])).double()


def border_is_zero(buf, H, W):
    b = buf.reshape(-1, H + 2, W + 2, 8)
    return all(float(e.abs().max()) == 0.0 for e in (b[:, 0], b[:, -1], b[:, :, 0], b[:, :, -1]))


def run_engine_encoder(lib, dev, prob, variant):
    """prob: a fit problem dict (model, vposer_w, enc_w, ids, Xmean, Xstd, seq, markers_rec, B); the image is H = 3 n81 + 2 by W = B + 15.
    Forward: every act[l] against float64 layers applied to the engine's own x0.  Backward: dx0 against float64 backward-data from the
    smoothness loss's d(pre-act 10), through the engine's own LeakyReLU decisions (the signs of its saved activations): where a float64
    pre-activation and the fp32 one straddle zero, a float64 chain's gradient differs by O(1) there, not by rounding."""
    from lemo_amd.fitting import AmassTemporalFitter
    from lemo_amd.priors import ENC_CHANNELS
    A = prob['enc_w']
    B = prob['B']
    fit = AmassTemporalFitter(prob['model'], prob['vposer_w'], A, prob['ids'], prob['Xmean'], prob['Xstd'], B, dev, full_vertices=True,
                              conv_variant=variant, lib=lib)
    assert fit.conv_variant == variant
    fit.load_sequence(prob['seq']['init_params'], prob['markers_rec'], prob['seq']['contact_lbl'])
    fit.forward()
    fit.backward()
    _sync(lib)
    H, W = fit.H, fit.W
    what = f'fit engine, conv variant {variant}, {H} x {W}'
    x0 = fit.ws['x0'].cpu().view(H + 2, W + 2).double()
    assert float(x0.abs().max()) > 0, what
    h = x0[1:-1, 1:-1][None, None]
    keys = enc_layer_keys()
    for l, k in enumerate(keys):
        h = F.leaky_relu(F.conv2d(h, _w64(A, k), torch.from_numpy(np.asarray(A[k + '.bias'])).double(), padding=1), SLOPE)
        got = from_cg8p(fit.act[l + 1].cpu(), H, W).double()
        e = float((got - h[0]).abs().max() / h.abs().max())
        Rec.add('enc_act', e, e)
        assert e < ENC_ACT_REL, f'{what}: act[{l + 1}] ({ENC_CHANNELS[l + 1]} ch) {e:.3e}'
        assert border_is_zero(fit.act[l + 1].cpu(), H, W), f'{what}: act[{l + 1}] border'
    # d(smooth loss)/d(pre-act 10), smooth loss = w mean((z[..., 1:] - z[..., :-1])^2) over 64 H (W - 1) terms (opt_amass_temp.py:390-391)
    z = from_cg8p(fit.act[10].cpu(), H, W).double()
    dz = torch.zeros_like(z)
    dd = z[..., 1:] - z[..., :-1]
    dz[..., 1:] += dd
    dz[..., :-1] -= dd
    d = (dz * (2.0 * fit.weights['smooth'] / (64 * H * (W - 1))) * lrelu_d(z))[None]
    for l in range(9, 0, -1):
        d = F.conv_transpose2d(d, _w64(A, keys[l]), padding=1) * lrelu_d(from_cg8p(fit.act[l].cpu(), H, W))[None]
    ref = F.conv_transpose2d(d, _w64(A, keys[0]), padding=1)[0, 0]
    dx = fit.ws['dx0'].cpu().view(H, W).double()
    e = float((dx - ref).abs().max() / ref.abs().max())
    Rec.add('enc_dx0', e, e)
    assert e < ENC_DX0_REL, f'{what}: dx0 {e:.3e}'
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# the infilling AE's convolutions (lemo_ae_conv: fp32 operands; lemo_ae_conv_f16: two fp16 pieces per operand, scales from tensor maxima)

def _ae_launch(lib, f16, x, wt, bias, aux, out, H, W, fH, fW, in_s, out_s, cin, cout, epi, geo, s, amax_in=None, wmax=None, amax_out=None):
    mt, pt, ks = geo
    if f16:
        return lib.ae_conv_f16(ptr(x), ptr(wt), ptr(bias), ptr(aux), ptr(out), H, W, fH, fW, in_s, out_s, cin, cout, epi, mt, pt, ks,
                               ptr(amax_in), 1.0, ptr(wmax), ptr(amax_out), s)
    return lib.ae_conv(ptr(x), ptr(wt), ptr(bias), ptr(aux), ptr(out), H, W, fH, fW, in_s, out_s, cin, cout, epi, mt, pt, ks, s)


def run_ae_conv(lib, dev, f16, H, W, cin, cout, geo, fine=None):
    """plain geometry, epilogues 0 / 1 (conv x lrelu'(aux): the engine passes backward packs itself) / 2; with fine = (fH, fW), where
    H x W is the max-pooled size of fH x fW, also the zero-stuffing output (even pixels of the fine image) and the strided input"""
    arith = 'ae_f16' if f16 else 'fp32'
    kname = 'ae_conv_f16' if f16 else 'ae_conv'
    g = torch.Generator().manual_seed(H * 131 + W * 7 + cin + cout + sum(geo))
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    wt, bd = torch.from_numpy(pack_conv3x3(w.numpy())).to(dev), b.to(dev)
    wmax = w.abs().max().reshape(1).to(dev)
    s = _stream(lib, dev)

    def launch(xin, xmax, aux, out, Hq, Wq, fH, fW, in_s, out_s, epi):
        amax_out = torch.zeros(1, device=dev)
        rc = _ae_launch(lib, f16, xin, wt, None if epi == 1 else bd, aux, out, Hq, Wq, fH, fW, in_s, out_s, cin, cout, epi, geo, s,
                        xmax.reshape(1).to(dev), wmax, amax_out)
        return rc, amax_out

    if geo[0] == 2 and cout % 64:                # 32 px x 64 cout tiles need cout % 64 == 0: LEMO_ERR_ARG, nothing written
        whole, o = sentinel_cg8p(cout, H, W, dev)
        x = torch.randn(cin, H, W, generator=g)
        rc, _ = launch(to_cg8p(x).to(dev), x.abs().max(), None, o, H, W, 0, 0, 1, 1, 0)
        _sync(lib)
        assert rc == ERR_ARG and torch.isnan(whole.cpu()).all(), f'{kname} {geo} {cin}->{cout}: rc {rc}'
        return
    for epi in (0, 1, 2):
        what = f'{kname} {geo} epi {epi} {cin}->{cout} at {H} x {W}'
        x = torch.randn(cin, H, W, generator=g) * (1e-6 if epi == 1 else 0.5)
        aux = torch.randn(cout, H, W, generator=g)
        xd = x[None].double()
        pre = F.conv2d(xd, w.double(), None if epi == 1 else b.double(), padding=1)[0]
        mag = F.conv2d(xd.abs(), w.double().abs(), None if epi == 1 else b.double().abs(), padding=1)[0]
        if epi == 1:
            ref, mag = pre * lrelu_d(aux), mag * lrelu_d(aux)
        else:
            ref = F.leaky_relu(pre, SLOPE) if epi == 0 else pre
        xin, auxp = to_cg8p(x).to(dev), to_cg8p(aux).to(dev)
        outs = []
        for _ in range(2):
            whole, o = sentinel_cg8p(cout, H, W, dev)
            rc, amax_out = launch(xin, x.abs().max(), auxp, o, H, W, 0, 0, 1, 1, epi)
            lib.check(rc, what)
            outs.append((whole, o, amax_out))
        _sync(lib)
        (w1, o1, am1), (w2, _, _) = outs
        check_cg8p_write_set(w1, cout, H, W, what)
        same_bits(w1, w2, what)
        got = from_cg8p(o1.cpu(), H, W)
        check_close(got, ref, mag, arith, what)
        if f16:
            assert float(am1.cpu()) == float(got.abs().max()), what + ': amax_out is not max |out|'
    if fine is None:
        return
    fH, fW = fine
    assert (fH - 1) // 2 + 1 == H and (fW - 1) // 2 + 1 == W
    # zero-stuffing output: lrelu(conv + b) at (2y, 2x) of the fine image, zero at the other fine pixels (interior pre-zeroed, border NaN)
    what = f'{kname} {geo} stuffed output {H} x {W} -> {fH} x {fW}'
    x = torch.randn(cin, H, W, generator=g) * 0.5
    ref, mag = ref_layer(x, w, b, 0)
    whole, o = sentinel_cg8p(cout, fH, fW, dev)
    o.view(cout // 8, fH + 2, fW + 2, 8)[:, 1:-1, 1:-1] = 0.0
    rc, _ = launch(to_cg8p(x).to(dev), x.abs().max(), None, o, H, W, fH, fW, 1, 2, 0)
    lib.check(rc, what)
    _sync(lib)
    check_cg8p_write_set(whole, cout, fH, fW, what)
    S = from_cg8p(o.cpu(), fH, fW)
    check_close(S[:, 0::2, 0::2], ref, mag, arith, what)
    assert float(S[:, 1::2].abs().max()) == 0.0 and float(S[:, :, 1::2].abs().max()) == 0.0, what + ': odd fine pixels written'
    # strided input: conv of the fine image at its even pixels x lrelu'(aux read at the same even pixels)
    what = f'{kname} {geo} strided input {fH} x {fW} -> {H} x {W}'
    xf = torch.randn(cin, fH, fW, generator=g) * 1e-6
    aux = torch.randn(cout, H, W, generator=g)
    auxf = torch.zeros(cout, fH, fW)
    auxf[:, 0::2, 0::2] = aux
    ref = F.conv2d(xf[None].double(), w.double(), padding=1)[0, :, 0::2, 0::2] * lrelu_d(aux)
    mag = F.conv2d(xf[None].double().abs(), w.double().abs(), padding=1)[0, :, 0::2, 0::2] * lrelu_d(aux)
    whole, o = sentinel_cg8p(cout, H, W, dev)
    rc, _ = launch(to_cg8p(xf).to(dev), xf.abs().max(), to_cg8p(auxf).to(dev), o, H, W, fH, fW, 2, 1, 1)
    lib.check(rc, what)
    _sync(lib)
    check_cg8p_write_set(whole, cout, H, W, what)
    check_close(from_cg8p(o.cpu(), H, W), ref, mag, arith, what)
