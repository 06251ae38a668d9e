"""Direct tests of the small kernels that sit under both engines, through their own C entry points, against float64 on the CPU
(tests/test_blocks_emu.py on the host-emulated build, tests/test_blocks_gpu.py on the MI355X; both run the cases below):

  lemo_gemm_nt16                      the VPoser MLP GEMM, four epilogues                       csrc/gemm_kernels.hip
  lemo_gemm_nt16_splitk               its long-K form on the bf16 matrix cores                  csrc/gemm_kernels.hip
  lemo_maxpool3s2_fwd / _bwd          MaxPool2d(3, 2, 1) with winner bytes                      csrc/ae_kernels.hip
  lemo_stuff2_fwd / _bwd              zero-stuffing of a stride-2 transposed convolution        csrc/ae_kernels.hip
  lemo_conv3x3_wgrad, _partial, _reduce_multi      the AE's weight gradient                     csrc/ae_kernels.hip
  lemo_sdf_sample                     trilinear SDF lookup == F.grid_sample(border, align_corners=False)   csrc/scene_device.hpp

The shapes are the smallest at which each code path exists (an idle K-split wave, a second round of chunks, an empty slab, a
slab shorter than the look-ahead, a ragged channel tile, the 512-pixel slab edge, W = 1, ...), not workload shapes.

Tolerances
----------
* GEMMs and the weight gradient (results with rounding freedom).  err(v) = max |v - ref| / max |ref| against the float64 result
  formed from the same float32 inputs.  The yardstick is a float32 CPU restatement of the same operation (torch float32 matmul /
  autograd of float32 F.conv2d / a float32 sum): the kernel may be at most GATE = 4 times as far from float64 as the restatement is.
  Only where the restatement's own error is exactly zero (a one-pixel image: every entry is a single product) the kernel gets the
  floor 2^-23, one ulp of the largest entry.  The split-K GEMM keeps its earlier absolute bound of 2e-6 as well.  The measured
  ratios are collected in RATIOS and printed by the last test of either module (DESIGN.md quotes them).
* Pooled values, winner bytes, the zero-stuffed image and the stuffing gather have no rounding freedom: equal bits.  A winner is the
  first maximum of the window in row-major order (torch's rule); the tied data set ({-1, 0, 1}) makes that rule decide most windows,
  which is checked on the CPU before the kernel runs.
* Pooling backward: a pixel collects the gradient of the <= 4 windows it won.  With <= 1 contribution the result is that float (times
  the float32 lrelu' factor where `act` is given: one IEEE product, the same on every machine): equal bits.  With 2 .. 4 contributions
  the float32 sum may be taken in any order: |got - ref| <= 3 * 2^-24 * sum |terms| (the bound of a 4-term float32 sum: three
  additions, each within 2^-24 of its partial sum <= sum |terms|), times the factor, plus 2^-24 |ref| for the product's rounding
  where `act` is given.
* sdf_sample.  Let u = 2^-24 and S = max |sdf|.  The voxel coordinate of an axis of size n comes from five float32 operations on
  numbers of size <= n, so it is within 5 u n of the float64 one; moving a coordinate by d moves the value by <= 2 S d (neighbouring
  voxels differ by <= 2 S), and the seven interpolations add <= 24 u S: |value - ref| <= u S (10 (D + H + W) + 24).  A gradient
  component is a difference of voxels (<= 2 S) interpolated along the two OTHER axes, times m = size / (gmax - gmin): within
  m u S (20 (sum of the other two sizes) + 24).  It is discontinuous where the point crosses a voxel centre of its own axis, so the
  random points are drawn >= 0.05 voxels from every centre (checked on the CPU, beforehand); where the centres are exact in both
  precisions (the 1 x 4 x 4 volume in a power-of-two box) points ON them are compared directly, and in the 5 x 6 x 7 volume a
  component at a nominal centre may equal the float64 slope of either side of its own axis' centre.  A clamped axis has gradient exactly 0, including a
  point exactly on the first or last voxel centre (torch's clip_coordinates_set_grad).

Buffers: every input region the contract says is never read holds NaN (columns K.. of A and B, columns M.. of C and aux, the whole
split-K workspace); every output sits between GUARD sentinel elements and is pre-filled with NaN where it must not be written
(stride padding; rows >= N are the guard itself).  CG8P borders are real zero padding: they are zero before and must be zero after."""
import ctypes as C

import torch
import torch.nn.functional as F

from lemo_amd._hip import WgradJob, ptr
from lemo_amd.priors import from_cg8p, to_cg8p

ERR_SHAPE = 10001
ERR_ARG = 10002
SLOPE = 0.2                       # LEMO_LRELU_SLOPE
SLOPE32 = torch.tensor(0.2, dtype=torch.float32)
GUARD = 64                        # sentinel elements before and after every output (a multiple of 4: 16-byte alignment is kept)
GATE = 4.0
FLOOR = 2.0 ** -23
U = 2.0 ** -24
NAN = float('nan')

RATIOS = {}                       # family -> (worst kernel error / restatement error, worst kernel error, cases counted)


def _sync(lib):
    if not lib.is_emu:
        torch.cuda.synchronize()


def guarded(n, dev, dtype=torch.float32, fill=NAN):
    """(whole, view): n elements between two runs of GUARD sentinels, the view pre-filled with `fill`"""
    sent = NAN if dtype == torch.float32 else 0xAB
    whole = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    view = whole[GUARD:GUARD + n]
    view.fill_(fill)
    return whole, view


def guards_intact(whole, n, what):
    w = whole.cpu()
    g = torch.cat([w[:GUARD], w[GUARD + n:]])
    ok = torch.isnan(g).all() if w.dtype == torch.float32 else (g == 0xAB).all()
    assert ok, f'{what}: wrote outside its buffer'
    return w[GUARD:GUARD + n]


def guarded_cg8p(Cn, H, W, dev):
    """CG8P output [C/8][(H+2)(W+2)][8]: zero border, NaN interior, guards around it"""
    n = (Cn // 8) * (H + 2) * (W + 2) * 8
    whole, view = guarded(n, dev, fill=0.0)
    view.view(Cn // 8, H + 2, W + 2, 8)[:, 1:-1, 1:-1, :] = NAN
    return whole, view


def cg8p_result(whole, Cn, H, W, what):
    """guards intact, border still zero, interior finite -> [C, H, W]"""
    n = (Cn // 8) * (H + 2) * (W + 2) * 8
    b = guards_intact(whole, n, what).view(Cn // 8, H + 2, W + 2, 8)
    inner = torch.zeros(H + 2, W + 2, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    assert (b[:, ~inner].view(torch.int32) == 0).all(), f'{what}: wrote into the zero border'
    assert torch.isfinite(b[:, inner]).all(), f'{what}: left interior pixels unwritten (or non-finite)'
    return from_cg8p(b.reshape(Cn // 8, (H + 2) * (W + 2), 8), H, W)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


def err_of(v, ref):
    return float((v.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def gate(family, got, f32, ref, what):
    """the kernel against the float32 restatement's own distance from float64"""
    assert torch.isfinite(got).all(), what
    e_k, e_32 = err_of(got, ref), err_of(f32, ref)
    bound = GATE * e_32 if e_32 > 0 else FLOOR
    ratio = e_k / e_32 if e_32 > 0 else 0.0
    r, e, n = RATIOS.get(family, (0.0, 0.0, 0))
    RATIOS[family] = (max(r, ratio), max(e, e_k), n + 1)
    print(f'{what}: kernel {e_k:.3e} restatement {e_32:.3e} ratio {ratio:.2f}')
    assert e_k <= bound, f'{what}: {e_k:.3e} from float64, the float32 restatement {e_32:.3e} (gate {GATE:g} x, floor {FLOOR:.1e} at zero)'
    return e_k


def report_ratios():
    for k in sorted(RATIOS):
        r, e, n = RATIOS[k]
        print(f'blocks ratio {k}: worst kernel / restatement {r:.2f}, worst kernel error {e:.3e} ({n} comparisons)')
    assert RATIOS, 'no case ran before the report'


def lrelu_d32(act):
    return torch.where(act > 0, torch.ones((), dtype=torch.float32), SLOPE32)


# ---------------------------------------------------------------------------------------------------------------------------
# lemo_gemm_nt16: C[n][m] = epi(sum_k A[m][k] B[n][k]); four waves split K/16 chunks (per = ceil(k16 / 4)), rounds of 8 chunks

GEMM_SHAPES = [                   # (M, N, K): every K with both M and >= 2 N; K = 16: three idle waves, 64: one chunk per wave,
    (16, 1, 16), (48, 17, 16),    # 80: k16 = 5, per = 2, wave 3 starts past the end, 528: per = 9 (second round of one chunk),
    (16, 15, 64), (48, 16, 64),   # 1040: per = 17 (three rounds)
    (16, 33, 80), (48, 1, 80), (16, 17, 80),
    (16, 17, 528), (48, 15, 528),
    (16, 16, 1040), (48, 33, 1040),
]
GEMM_EPIS = (0, 1, 2, 3)


def _padded(rows, cols, ld, g, scale=1.0):
    """[rows][ld] float32 with NaN in columns cols .. ld - 1"""
    t = torch.full((rows, ld), NAN)
    t[:, :cols] = torch.randn(rows, cols, generator=g) * scale
    return t


def gemm_inputs(M, N, K, tight, seed):
    g = torch.Generator().manual_seed(seed)
    lda, ldb, ldc, ldaux = (K, K, M, M) if tight else (K + 4, K + 8, M + 4, M + 12)
    A, B = _padded(M, K, lda, g), _padded(N, K, ldb, g, 0.5)
    bias = torch.randn(M, generator=g)
    aux = _padded(N, M, ldaux, g)
    aux[:, :M][torch.rand(N, M, generator=g) < 0.25] = 0.0           # positive, negative and exactly-zero entries
    return A, B, bias, aux, (lda, ldb, ldc, ldaux)


def gemm_reference(A, B, bias, aux, M, K, epi, dtype):
    a, b = A[:, :K].to(dtype), B[:, :K].to(dtype)
    v = b @ a.t()
    if epi == 1:
        return F.leaky_relu(v + bias.to(dtype), SLOPE)
    if epi == 2:
        return v + bias.to(dtype)
    if epi == 3:
        return v * torch.where(aux[:, :M] > 0, 1.0, SLOPE).to(dtype)
    return v


def check_gemm(lib, dev, M, N, K, epi, tight=False):
    A, B, bias, aux, (lda, ldb, ldc, ldaux) = gemm_inputs(M, N, K, tight, seed=M * 7 + N * 131 + K + epi)
    a3 = aux[:, :M]
    assert epi != 3 or ((a3 > 0).any() and (a3 < 0).any() and (a3 == 0).any())
    ref = gemm_reference(A, B, bias, aux, M, K, epi, torch.float64)
    f32 = gemm_reference(A, B, bias, aux, M, K, epi, torch.float32)
    Ad, Bd, bd, auxd = A.to(dev), B.to(dev), bias.to(dev), aux.to(dev)
    whole, Cv = guarded(N * ldc, dev)
    rc = lib.gemm_nt16(ptr(Ad), lda, ptr(Bd), ldb, M, N, K, ptr(Cv), ldc, ptr(bd) if epi in (1, 2) else None,
                       ptr(auxd) if epi == 3 else None, ldaux, epi, lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    what = f'gemm_nt16 epi {epi} M {M} N {N} K {K}' + (' tight' if tight else '')
    Cm = guards_intact(whole, N * ldc, what).view(N, ldc)
    assert torch.isnan(Cm[:, M:]).all(), f'{what}: wrote into the stride padding of C'
    gate('gemm_nt16', Cm[:, :M], f32, ref, what)


def check_gemm_refusals(lib, dev):
    M, N, K = 16, 3, 16
    A, B = torch.randn(32, 40).to(dev), torch.randn(N, 40).to(dev)
    bias, aux = torch.randn(32).to(dev), torch.randn(N, 32).to(dev)
    s = lib.stream(dev)
    cases = [                     # (M, K, lda, ldb, ldc, bias, aux, ldaux, epi, code)
        (24, K, 40, 40, 32, None, None, 32, 0, ERR_SHAPE),             # M not a multiple of 16
        (M, 24, 40, 40, 32, None, None, 32, 0, ERR_SHAPE),             # K not a multiple of 16
        (M, K, 38, 40, 32, None, None, 32, 0, ERR_SHAPE),              # strides not multiples of 4
        (M, K, 40, 38, 32, None, None, 32, 0, ERR_SHAPE),
        (M, K, 40, 40, 30, None, None, 32, 0, ERR_SHAPE),
        (M, K, 40, 40, 32, bias, aux, 32, 4, ERR_ARG),                 # no such epilogue
        (M, K, 40, 40, 32, None, aux, 32, 1, ERR_ARG),                 # bias epilogues without bias
        (M, K, 40, 40, 32, None, aux, 32, 2, ERR_ARG),
        (M, K, 40, 40, 32, bias, None, 32, 3, ERR_ARG),                # lrelu' epilogue without aux
    ]
    for m, k, lda, ldb, ldc, b_, a_, ldaux, epi, code in cases:
        whole, Cv = guarded(N * 32, dev)
        rc = lib.gemm_nt16(ptr(A), lda, ptr(B), ldb, m, N, k, ptr(Cv), ldc, ptr(b_), ptr(a_), ldaux, epi, s)
        _sync(lib)
        assert rc == code, (m, k, lda, ldb, ldc, epi, rc)
        assert torch.isnan(whole.cpu()).all(), f'refused gemm_nt16 (epi {epi}) wrote its output'


# ---------------------------------------------------------------------------------------------------------------------------
# lemo_gemm_nt16_splitk: S slabs of ceil(k16 / S) 16-k steps each, SK_RA = 3 steps of look-ahead, 64- or 128-row workgroups

SPLITK_M = (64, 128, 192)         # 64, 192: the 64-row workgroups; 128: the 128-row ones
SPLITK_N = (1, 37, 128)
SPLITK_KS = ((10, 7), (5, 5), (6, 3), (9, 1))    # (K / 16, S): slabs 5 and 6 empty | one-step slabs | two-step slabs | one slab


def check_splitk(lib, dev, M, N, k16, S):
    K = 16 * k16
    g = torch.Generator().manual_seed(M + 1000 * N + 7 * k16 + S)
    lda = ldb = K + 4
    ldc = M + 4
    A, B = _padded(M, K, lda, g), _padded(N, K, ldb, g, 0.5)
    ref = B[:, :K].double() @ A[:, :K].double().t()
    f32 = B[:, :K] @ A[:, :K].t()
    Ag = A[:, :K].reshape(M, k16, 16).permute(1, 0, 2).contiguous()     # [K/16][M][16]
    Ad, Bd, Agd = A.to(dev), B.to(dev), Ag.to(dev)
    npart = lib.gemm_nt16_splitk_part_floats(M, S)
    assert npart == S * 128 * M
    what = f'gemm_nt16_splitk M {M} N {N} K {K} S {S}'
    outs = []
    for grouped in (False, False, True):
        pwhole, part = guarded(npart, dev)                                # the workspace holds NaN before the call
        whole, Cv = guarded(N * ldc, dev)
        rc = lib.gemm_nt16_splitk(ptr(Ad), lda, ptr(Bd), ldb, M, N, K, ptr(Cv), ldc, ptr(part), S, ptr(Agd) if grouped else None,
                                  lib.stream(dev))
        _sync(lib)
        assert rc == 0, rc
        guards_intact(pwhole, npart, what + ' (part)')
        Cm = guards_intact(whole, N * ldc, what).view(N, ldc)
        assert torch.isnan(Cm[:, M:]).all(), f'{what}: wrote into the stride padding of C'
        assert torch.isfinite(Cm[:, :M]).all(), f'{what}: unwritten or non-finite outputs (grouped {grouped})'
        outs.append(Cm[:, :M].clone())
    same_bits(outs[0], outs[1], f'{what}: two runs differ')
    same_bits(outs[0], outs[2], f'{what}: A_grouped differs from row-major A')
    e = gate('gemm_nt16_splitk', outs[0], f32, ref, what)
    assert e < 2e-6, f'{what}: {e:.3e} >= 2e-6'


def check_splitk_refusals(lib, dev):
    K = 64
    A, B = torch.randn(192, K).to(dev), torch.randn(130, K).to(dev)
    part = torch.zeros(lib.gemm_nt16_splitk_part_floats(192, 8)).to(dev)
    for M, N, S in ((64, 129, 2), (32, 8, 2), (64, 8, 0), (64, 8, K // 16 + 1)):
        whole, Cv = guarded(130 * 192, dev)
        rc = lib.gemm_nt16_splitk(ptr(A), K, ptr(B), K, M, N, K, ptr(Cv), M, ptr(part), S, None, lib.stream(dev))
        _sync(lib)
        assert rc == ERR_SHAPE, (M, N, S, rc)
        assert torch.isnan(whole.cpu()).all(), 'refused gemm_nt16_splitk wrote its output'


# ---------------------------------------------------------------------------------------------------------------------------
# MaxPool2d(3, 2, 1) forward / backward

POOL_C = (8, 24)
POOL_HW = ((1, 1), (1, 6), (6, 1), (2, 2), (7, 10), (9, 33))
POOL_KINDS = ('random', 'tied')


def pool_input(Cn, H, W, kind, seed):
    """a LeakyReLU-output-like image [C, H, W] with exact zeros; 'tied': {-1, 0, 1}, mostly 1, so that most windows tie at the maximum"""
    g = torch.Generator().manual_seed(seed)
    if kind == 'tied':
        r = torch.rand(Cn, H, W, generator=g)
        return torch.where(r < 0.6, 1.0, torch.where(r < 0.8, 0.0, -1.0)).float()
    x = F.leaky_relu(torch.randn(Cn, H, W, generator=g), SLOPE)
    x[torch.rand(Cn, H, W, generator=g) < 0.1] = 0.0
    return x


def pool_first_max(x):
    """(values [C, Ho, Wo], tap [C, Ho, Wo], ties [C, Ho, Wo]): the first maximum of every window in row-major window order"""
    Cn, H, W = x.shape
    cols = F.unfold(F.pad(x[None], (1, 1, 1, 1), value=float('-inf')), 3, stride=2)[0].view(Cn, 9, -1)      # [C, 9, Ho*Wo]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    vmax = cols.max(1).values
    is_max = cols == vmax[:, None]
    tap = (is_max.int() * torch.arange(9, 0, -1).view(1, 9, 1)).argmax(1)            # first True: the largest weight 9 - tap
    return vmax.view(Cn, Ho, Wo), tap.view(Cn, Ho, Wo), (is_max.sum(1) > 1).view(Cn, Ho, Wo)


def check_pool(lib, dev, Cn, H, W, kind):
    x = pool_input(Cn, H, W, kind, seed=Cn * 100 + H * 37 + W)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    vals, tap, ties = pool_first_max(x)
    xr = x.double().requires_grad_(True)
    ref, ridx = F.max_pool2d(xr[None], 3, 2, 1, return_indices=True)
    ry, rx = ridx[0] // W, ridx[0] % W                                   # torch's winner as a tap of the same window
    yo, xo = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing='ij')
    assert torch.equal((ry - (2 * yo - 1)) * 3 + (rx - (2 * xo - 1)), tap), 'torch does not route to the first maximum'
    if kind == 'tied' and H * W > 1:
        assert float(ties.float().mean()) > 0.5, f'the tied data ties in only {float(ties.float().mean()):.2f} of the windows'
    if kind == 'random' and H * W > 1:
        assert (x == 0).any() and (x > 0).any() and (x < 0).any()
    what = f'maxpool3s2 C {Cn} {H} x {W} {kind}'
    s = lib.stream(dev)
    xb = to_cg8p(x).to(dev)
    owhole, out = guarded_cg8p(Cn, Ho, Wo, dev)
    iwhole, idx = guarded((Cn // 8) * Ho * Wo * 8, dev, dtype=torch.uint8, fill=0xCD)
    rc = lib.maxpool3s2_fwd(ptr(xb), H, W, ptr(out), ptr(idx), Cn, s)
    _sync(lib)
    assert rc == 0, rc
    same_bits(cg8p_result(owhole, Cn, Ho, Wo, what + ' fwd'), vals, f'{what}: pooled values')
    same_bits(vals, ref[0].detach().float(), f'{what}: reference values')
    got_tap = guards_intact(iwhole, (Cn // 8) * Ho * Wo * 8, what + ' idx').view(Cn // 8, Ho, Wo, 8).permute(0, 3, 1, 2).reshape(Cn, Ho, Wo)
    assert torch.equal(got_tap.long(), tap), f'{what}: winner bytes are not the first maximum ({int((got_tap.long() != tap).sum())} differ)'
    # backward: gradient, |gradient| and the number of contributions per pixel from float64 autograd (same routing)
    g = torch.Generator().manual_seed(Cn + H + W)
    go = torch.randn(Cn, Ho, Wo, generator=g)
    gref, = torch.autograd.grad(ref, xr, go.double()[None], retain_graph=True)
    gabs, = torch.autograd.grad(ref, xr, go.double().abs()[None], retain_graph=True)
    cnt, = torch.autograd.grad(ref, xr, torch.ones_like(ref))
    single = cnt <= 1
    if H * W >= 70:
        assert (cnt >= 2).any(), 'no pixel wins two windows: the summed path is not exercised'
    gob = to_cg8p(go).to(dev)
    for use_act in (False, True):
        fac = lrelu_d32(x) if use_act else torch.ones_like(x)
        dwhole, din = guarded_cg8p(Cn, H, W, dev)
        rc = lib.maxpool3s2_bwd(ptr(gob), ptr(idx), ptr(xb) if use_act else None, ptr(din), H, W, Cn, s)
        _sync(lib)
        assert rc == 0, rc
        got = cg8p_result(dwhole, Cn, H, W, f'{what} bwd act {use_act}')
        exact = gref.float() * fac                                        # one float (or 0) times the float32 factor
        same_bits(got[single] + 0.0, exact[single] + 0.0, f'{what} bwd act {use_act}: single-window pixels')
        refd = gref * fac.double()
        tol = 3 * U * gabs * fac.double() + (U * refd.abs() if use_act else 0.0)
        bad = (got.double() - refd).abs() > tol
        assert not bad[~single].any(), f'{what} bwd act {use_act}: {int(bad.sum())} summed pixels outside 3 * 2^-24 * sum |terms|'


def check_pool_refusals(lib, dev):
    Cn, H, W = 12, 4, 4
    xb = torch.zeros(2, 36, 8).to(dev)
    whole, out = guarded(2 * 16 * 8, dev)
    iwhole, idx = guarded(2 * 4 * 8, dev, dtype=torch.uint8, fill=0xAB)
    assert lib.maxpool3s2_fwd(ptr(xb), H, W, ptr(out), ptr(idx), Cn, lib.stream(dev)) == ERR_SHAPE
    dwhole, din = guarded(2 * 36 * 8, dev)
    assert lib.maxpool3s2_bwd(ptr(out), ptr(idx), None, ptr(din), H, W, Cn, lib.stream(dev)) == ERR_SHAPE
    _sync(lib)
    assert torch.isnan(whole.cpu()).all() and torch.isnan(dwhole.cpu()).all() and (iwhole.cpu() == 0xAB).all()


# ---------------------------------------------------------------------------------------------------------------------------
# zero-stuffing of ConvTranspose2d(stride 2, output_size = H x W) and its adjoint

STUFF_C = 16
STUFF_CASES = (((1, 1), (1, 1)), ((1, 1), (2, 2)), ((4, 5), (7, 9)), ((4, 5), (8, 10)), ((4, 5), (7, 10)))


def check_stuff(lib, dev, h, w, H, W):
    Cn = STUFF_C
    g = torch.Generator().manual_seed(h * 1000 + w * 100 + H * 10 + W)
    z = torch.randn(Cn, h, w, generator=g)
    what = f'stuff2 {h} x {w} -> {H} x {W}'
    s = lib.stream(dev)
    want = torch.zeros(Cn, H, W)
    want[:, ::2, ::2][:, :h, :w] = z
    zb = to_cg8p(z).to(dev)
    owhole, out = guarded_cg8p(Cn, H, W, dev)
    rc = lib.stuff2_fwd(ptr(zb), h, w, ptr(out), H, W, Cn, s)
    _sync(lib)
    assert rc == 0, rc
    same_bits(cg8p_result(owhole, Cn, H, W, what + ' fwd'), want, f'{what}: not the zero-stuffed image')
    go = torch.randn(Cn, H, W, generator=g)
    act = F.leaky_relu(torch.randn(Cn, h, w, generator=g), SLOPE)
    act[torch.rand(Cn, h, w, generator=g) < 0.3] = 0.0
    if h * w > 1:
        assert (act == 0).any() and (act > 0).any() and (act < 0).any()
    else:
        act[: Cn // 2] = 0.0
    gob, actb = to_cg8p(go).to(dev), to_cg8p(act).to(dev)
    for use_act in (False, True):
        dwhole, din = guarded_cg8p(Cn, h, w, dev)
        rc = lib.stuff2_bwd(ptr(gob), H, W, ptr(actb) if use_act else None, ptr(din), h, w, Cn, s)
        _sync(lib)
        assert rc == 0, rc
        gather = go[:, ::2, ::2][:, :h, :w]
        same_bits(cg8p_result(dwhole, Cn, h, w, f'{what} bwd act {use_act}'), gather * lrelu_d32(act) if use_act else gather,
                  f'{what} bwd act {use_act}: not the gather')


def check_stuff_refusals(lib, dev):
    Cn = STUFF_C
    zb, gob = torch.zeros(2, 7 * 7, 8).to(dev), torch.zeros(2, 9 * 11, 8).to(dev)
    for (h, w), (H, W) in (((5, 5), (7, 9)), ((4, 6), (7, 9)), ((2, 1), (1, 1))):       # 2 (h - 1) > H - 1 or 2 (w - 1) > W - 1
        owhole, out = guarded(2 * 9 * 11 * 8, dev)
        assert lib.stuff2_fwd(ptr(zb), h, w, ptr(out), H, W, Cn, lib.stream(dev)) == ERR_SHAPE, (h, w, H, W)
        dwhole, din = guarded(2 * 7 * 8 * 8, dev)
        assert lib.stuff2_bwd(ptr(gob), H, W, None, ptr(din), h, w, Cn, lib.stream(dev)) == ERR_SHAPE, (h, w, H, W)
        _sync(lib)
        assert torch.isnan(owhole.cpu()).all() and torch.isnan(dwhole.cpu()).all()
    owhole, out = guarded(2 * 9 * 11 * 8, dev)
    assert lib.stuff2_fwd(ptr(zb), 4, 5, ptr(out), 7, 9, 12, lib.stream(dev)) == ERR_SHAPE
    _sync(lib)
    assert torch.isnan(owhole.cpu()).all()


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradient of a 3 x 3 / stride-1 / pad-1 convolution: one call, and slab partials + the multi-job reduction

WGRAD_CH = ((8, 32, 4, 1), (8, 32, 8, 32), (40, 64, 40, 64), (64, 32, 64, 32))     # (cin, cout, cin_real, cout_real); 8, 40: ragged ci tile
WGRAD_HW = ((1, 1), (5, 1), (1, 5), (3, 2), (7, 16), (9, 15), (4, 32), (17, 31), (23, 23))
# H W = 1, 5, 5, 6 (< 16), 112, 135 (a ragged wave quarter of the 128-pixel quarters), 128, 527, 529 (around the 512-pixel slab); W = 1


def wgrad_inputs(cin, cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = F.leaky_relu(torch.randn(cin, H, W, generator=g), SLOPE)
    dy = torch.randn(cout, H, W, generator=g) * 0.1
    return x, dy


def wgrad_reference(x, dy, cin_real, cout_real, dtype):
    xd, gd = x[:cin_real].to(dtype)[None], dy[:cout_real].to(dtype)[None]
    w = torch.zeros(cout_real, cin_real, 3, 3, dtype=dtype, requires_grad=True)
    dw, = torch.autograd.grad(F.conv2d(xd, w, padding=1), w, gd)
    db = torch.zeros(cout_real, dtype=dtype)
    for col in gd[0].flatten(1).t():                                     # db[co] = sum_p dy[co][p] as a running sum in `dtype`, pixel order
        db = db + col                                                    # (torch.sum and cumsum accumulate float32 in wider or cascaded form)
    return dw, db


def _job(part, dyb, dw, db, nslab, cin, cout, cin_real, cout_real, H, W):
    return WgradJob(ptr(part), ptr(dyb), ptr(dw), ptr(db), nslab, cin, cout, cin_real, cout_real, H, W)


def run_wgrad_one_call(lib, dev, x, dy, cin_real, cout_real, what):
    """lemo_conv3x3_wgrad with guarded partial / dw / db -> (dw, db) on the CPU"""
    cin, H, W = x.shape
    cout = dy.shape[0]
    nslab = lib.conv3x3_wgrad_nslab(H, W)
    assert nslab == (H * W + 511) // 512
    xb, dyb = to_cg8p(x).to(dev), to_cg8p(dy).to(dev)
    npart, ndw = nslab * 9 * cout * cin, cout_real * cin_real * 9
    pwhole, part = guarded(npart, dev)
    wwhole, dw = guarded(ndw, dev)
    bwhole, db = guarded(cout_real, dev)
    rc = lib.conv3x3_wgrad(ptr(dyb), ptr(xb), H, W, cin, cout, cin_real, cout_real, ptr(part), ptr(dw), ptr(db), lib.stream(dev))
    _sync(lib)
    assert rc == 0, f'{what}: refused ({rc})'
    assert torch.isfinite(guards_intact(pwhole, npart, what + ' partial')).all(), f'{what}: unwritten slab partials'
    return (guards_intact(wwhole, ndw, what + ' dw').view(cout_real, cin_real, 3, 3).clone(),
            guards_intact(bwhole, cout_real, what + ' db').clone())


def run_wgrad_two_stage(lib, dev, jobs_in, what):
    """lemo_conv3x3_wgrad_partial per job, then ONE lemo_conv3x3_wgrad_reduce_multi -> [(dw, db or None)]"""
    s = lib.stream(dev)
    jobs = (WgradJob * len(jobs_in))()
    keep = []
    for k, (x, dy, cin_real, cout_real, want_db) in enumerate(jobs_in):
        cin, H, W = x.shape
        cout = dy.shape[0]
        nslab = lib.conv3x3_wgrad_nslab(H, W)
        xb, dyb = to_cg8p(x).to(dev), to_cg8p(dy).to(dev)
        npart, ndw = nslab * 9 * cout * cin, cout_real * cin_real * 9
        pwhole, part = guarded(npart, dev)
        wwhole, dw = guarded(ndw, dev)
        bwhole, db = guarded(cout_real, dev)
        assert lib.conv3x3_wgrad_partial(ptr(dyb), ptr(xb), H, W, cin, cout, ptr(part), s) == 0
        jobs[k] = _job(part, dyb, dw, db if want_db else None, nslab, cin, cout, cin_real, cout_real, H, W)
        keep.append((xb, dyb, pwhole, part, wwhole, dw, bwhole, db, npart, ndw, cout_real, cin_real, want_db))
    rc = lib.conv3x3_wgrad_reduce_multi(jobs, len(jobs_in), s)
    _sync(lib)
    assert rc == 0, rc
    out = []
    for k, (xb, dyb, pwhole, part, wwhole, dw, bwhole, db, npart, ndw, cout_real, cin_real, want_db) in enumerate(keep):
        assert torch.isfinite(guards_intact(pwhole, npart, f'{what} job {k} partial')).all()
        dwc = guards_intact(wwhole, ndw, f'{what} job {k} dw').view(cout_real, cin_real, 3, 3).clone()
        dbc = guards_intact(bwhole, cout_real, f'{what} job {k} db').clone()
        if not want_db:
            assert torch.isnan(dbc).all(), f'{what} job {k}: db written although the job has none'
        out.append((dwc, dbc if want_db else None))
    return out


def check_wgrad(lib, dev, cin, cout, cin_real, cout_real, H, W):
    what = f'conv3x3_wgrad {cin}({cin_real}) -> {cout}({cout_real}) {H} x {W}'
    x, dy = wgrad_inputs(cin, cout, H, W, seed=cin * 1000 + cout + H * 37 + W)
    ref_w, ref_b = wgrad_reference(x, dy, cin_real, cout_real, torch.float64)
    f32_w, f32_b = wgrad_reference(x, dy, cin_real, cout_real, torch.float32)
    dw, db = run_wgrad_one_call(lib, dev, x, dy, cin_real, cout_real, what)
    gate('conv3x3_wgrad dw', dw, f32_w, ref_w, what + ' dw')
    gate('conv3x3_wgrad db', db, f32_b, ref_b, what + ' db')
    (dw2, db2), = run_wgrad_two_stage(lib, dev, [(x, dy, cin_real, cout_real, True)], what)
    same_bits(dw2, dw, f'{what}: partial + reduce_multi dw differs from the one-call form')
    same_bits(db2, db, f'{what}: partial + reduce_multi db differs from the one-call form')


def check_wgrad_multi(lib, dev):
    """two jobs of different shapes in one reduction launch, the first without a bias gradient"""
    shapes = [((8, 32, 4, 1), (9, 15), False), ((40, 64, 40, 64), (23, 23), True)]
    jobs, one = [], []
    for (cin, cout, cr, cor), (H, W), want_db in shapes:
        x, dy = wgrad_inputs(cin, cout, H, W, seed=cin + cout + H + W)
        jobs.append((x, dy, cr, cor, want_db))
        one.append(run_wgrad_one_call(lib, dev, x, dy, cr, cor, f'wgrad_multi one-call {cin} -> {cout}'))
    for k, ((dw2, db2), (dw, db)) in enumerate(zip(run_wgrad_two_stage(lib, dev, jobs, 'wgrad_multi'), one)):
        same_bits(dw2, dw, f'wgrad_multi job {k}: dw')
        if db2 is not None:
            same_bits(db2, db, f'wgrad_multi job {k}: db')


def check_wgrad_refusals(lib, dev):
    s = lib.stream(dev)
    buf = torch.zeros(8 * 7 * 7 * 8).to(dev)
    whole, dw = guarded(64 * 64 * 9, dev)
    for cin, cout, cr, cor, H, W in ((12, 32, 12, 32, 5, 5), (8, 48, 8, 48, 5, 5), (8, 32, 9, 32, 5, 5), (8, 32, 8, 33, 5, 5), (8, 32, 8, 32, 0, 5),
                                     (8, 32, 8, 32, 5, 0)):
        assert lib.conv3x3_wgrad(ptr(buf), ptr(buf), H, W, cin, cout, cr, cor, ptr(buf), ptr(dw), None, s) == ERR_SHAPE, (cin, cout, cr, cor, H, W)
    assert lib.conv3x3_wgrad_partial(ptr(buf), ptr(buf), 5, 5, 12, 32, ptr(dw), s) == ERR_SHAPE
    jobs = (WgradJob * 1)()
    jobs[0] = _job(buf, buf, dw, None, lib.conv3x3_wgrad_nslab(23, 23) + 1, 8, 32, 8, 32, 23, 23)          # nslab is not the library's
    assert lib.conv3x3_wgrad_reduce_multi(jobs, 1, s) == ERR_SHAPE
    assert lib.conv3x3_wgrad_reduce_multi(jobs, 0, s) == ERR_ARG
    _sync(lib)
    assert torch.isnan(whole.cpu()).all(), 'a refused weight-gradient call wrote dw'


# ---------------------------------------------------------------------------------------------------------------------------
# lemo_sdf_sample

SDF_VOLUMES = {                   # name -> ((D, H, W), gmin, gmax); x <-> D, y <-> H, z <-> W
    '5x6x7': ((5, 6, 7), (-1.0, -1.1, -0.9), (1.0, 1.2, 1.1)),
    '1x4x4': ((1, 4, 4), (0.0, 0.0, 0.0), (1.0, 4.0, 4.0)),             # 2 / (gmax - gmin) is a power of two: voxel centres at k + 0.5 exactly
}
SDF_N = (1, 257)


def sdf_points(name, N, seed):
    """([N, 3] float32 points, [N] kind: 0 random inside, 1 outside / on the box faces, 2 on voxel centres)"""
    (D, H, W), gmin, gmax = SDF_VOLUMES[name]
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(gmin), torch.tensor(gmax)
    size = torch.tensor([D, H, W], dtype=torch.float32)
    # random points inside the box, by voxel coordinate: a cell (the outer half voxels included) plus a fraction in (0.05, 0.95), so
    # that no component sits on its gradient's discontinuity
    cell = torch.floor(torch.rand(N, 3, generator=g) * (size + 1)) - 1
    f = (cell + 0.05 + 0.9 * torch.rand(N, 3, generator=g)).clamp(-0.45, None).minimum(size - 0.55)
    pts = lo + (f + 0.5) / size * (hi - lo)
    if N == 1:
        return pts.float(), torch.zeros(1, dtype=torch.long)
    kind = torch.zeros(N, dtype=torch.long)
    k = 0
    for ax in range(3):                                                  # well outside on each side of each axis
        for side, off in ((lo, -0.7), (hi, 0.7), (lo, -40.0), (hi, 40.0)):
            pts[k, ax] = side[ax] + off * (hi[ax] - lo[ax])
            kind[k] = 1
            k += 1
    for ax in range(3):                                                  # exactly on gmin / gmax (one axis, then all three)
        for side in (lo, hi):
            pts[k, ax] = side[ax]
            kind[k] = 1
            k += 1
    pts[k], pts[k + 1] = lo, hi
    kind[k:k + 2] = 1
    k += 2
    cells = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij'), -1).view(-1, 3).float()
    cells = cells[torch.randperm(cells.shape[0], generator=g)[:min(64, cells.shape[0])]]
    n = cells.shape[0]
    pts[k:k + n] = lo + (cells + 0.5) / size * (hi - lo)                 # voxel centres (all three axes)
    kind[k:k + n] = 2
    k += n
    for ax in range(3):                                                  # a centre of ONE axis (first, last, middle), the rest random
        for c in (0, int(size[ax]) - 1, int(size[ax]) // 2):
            pts[k, ax] = lo[ax] + (c + 0.5) / size[ax] * (hi[ax] - lo[ax])
            kind[k] = 2
            k += 1
    assert k < N - 100
    return pts.float(), kind


def sdf_reference(sdf, pts, gmin, gmax, dtype):
    """(value [N], gradient [N, 3]) through F.grid_sample in `dtype`, from the same float32 points"""
    p = pts.to(dtype).requires_grad_(True)
    lo, hi = torch.tensor(gmin, dtype=torch.float32).to(dtype), torch.tensor(gmax, dtype=torch.float32).to(dtype)
    norm = (p - lo) / (hi - lo) * 2 - 1
    v = F.grid_sample(sdf.to(dtype)[None, None], norm[:, [2, 1, 0]].view(1, -1, 1, 1, 3), padding_mode='border', align_corners=False).view(-1)
    gr, = torch.autograd.grad(v.sum(), p)
    return v.detach(), gr


def check_sdf(lib, dev, name, N):
    (D, H, W), gmin, gmax = SDF_VOLUMES[name]
    g = torch.Generator().manual_seed(D * 100 + H * 10 + W)
    sdf = torch.randn(D, H, W, generator=g)
    pts, kind = sdf_points(name, N, seed=N + D)
    what = f'sdf_sample {name} N {N}'
    size = torch.tensor([D, H, W], dtype=torch.float64)
    lo, hi = torch.tensor(gmin, dtype=torch.float32).double(), torch.tensor(gmax, dtype=torch.float32).double()
    f = (pts.double() - lo) / (hi - lo) * size - 0.5                     # voxel coordinates in float64
    clamped = (f <= 0) | (f >= size - 1)
    off_centre = (f - f.round()).abs()
    rand = kind == 0
    assert (off_centre[rand] >= 1e-3).all(), 'a random point lies on a gradient discontinuity'
    if N > 1:
        assert (clamped[kind == 1].any(0)).all() and (~clamped[rand]).any(0)[size > 1].all() and clamped[rand].any(0).all()
    ref_v, ref_g = sdf_reference(sdf, pts, gmin, gmax, torch.float64)
    sd, pd = sdf.to(dev), pts.to(dev)
    vwhole, val = guarded(N, dev)
    gwhole, dval = guarded(3 * N, dev)
    g0, g1 = (C.c_float * 3)(*gmin), (C.c_float * 3)(*gmax)
    rc = lib.sdf_sample(ptr(sd), D, H, W, ptr(pd), N, g0, g1, ptr(val), ptr(dval), lib.stream(dev))
    _sync(lib)
    assert rc == 0, rc
    v = guards_intact(vwhole, N, what + ' val')
    gr = guards_intact(gwhole, 3 * N, what + ' dval').view(N, 3)
    assert torch.isfinite(v).all() and torch.isfinite(gr).all(), what
    S = float(sdf.abs().max())
    tol_v = U * S * (10 * (D + H + W) + 24)
    ev = (v.double() - ref_v).abs()
    print(f'{what}: value error {float(ev.max()):.3e} (bound {tol_v:.3e})')
    assert float(ev.max()) <= tol_v, f'{what}: value {float(ev.max()):.3e} > {tol_v:.3e}'
    # gradient: exactly 0 on a clamped axis; elsewhere within the derived bound of float64
    other = torch.tensor([H + W, D + W, D + H], dtype=torch.float64)
    tol_g = (size / (hi - lo)) * U * S * (20 * other + 24)
    eg = (gr.double() - ref_g).abs()
    on = torch.zeros_like(clamped)
    if name == '5x6x7':
        # the nominal centres are not exact here: component k may be the float64 slope of either side of its own axis' centre
        # (0 beside the first centre's outer side); the component is continuous in the other two axes, which stay where they are
        on = (kind == 2)[:, None] & (off_centre < 1e-4)
        d = 1e-3 * (hi - lo) / size
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                shifted = pts.double().clone()
                shifted[:, ax] += sgn * d[ax]
                _, g_side = sdf_reference(sdf, shifted, gmin, gmax, torch.float64)
                eg[:, ax] = torch.where(on[:, ax], torch.minimum(eg[:, ax], (gr[:, ax].double() - g_side[:, ax]).abs()), eg[:, ax])
    assert (gr[clamped & ~on] == 0).all(), f'{what}: nonzero gradient on a clamped axis'
    print(f'{what}: gradient error / bound {float((eg / tol_g).max()):.3f}')
    assert (eg <= tol_g).all(), f'{what}: gradient off by {float((eg / tol_g).max()):.2f} x its bound at point {int((eg / tol_g).max(1).values.argmax())}'
    # refusals
    assert lib.sdf_sample(ptr(sd), 0, H, W, ptr(pd), N, g0, g1, ptr(val), ptr(dval), lib.stream(dev)) == ERR_SHAPE
    assert lib.sdf_sample(ptr(sd), D, H, W, ptr(pd), 0, g0, g1, ptr(val), ptr(dval), lib.stream(dev)) == ERR_SHAPE
