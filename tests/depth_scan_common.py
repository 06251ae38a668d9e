"""Cases and yardsticks for lemo_amd.depth (csrc/depth_scan_kernels.hip), shared by tests/test_depth_scan_emu.py (host emulator) and
tests/test_depth_scan_gpu.py (MI355X).

Yardstick.  OpenCV is not part of this project's environment, so no fixture comes from the reference's own run.  ``restate`` is a
numpy restatement of temp_prox/projection_utils.py:35-90 plus OpenCV's documented model (5 undistortion iterations, Rodrigues,
projectPoints with k1 k2 p1 p2 k3), evaluated in float64 (the yardstick) and in plain float32 (the measure of what float32 costs).
Agreement with OpenCV itself is not confirmed by a run; ``roundtrip_residual`` prints how well project(undistort(pixel)) returns the
pixel, as a sanity check of the restatement alone (printed, not gated).  Nothing of the yardstick comes from lemo_amd.depth: the
undistortion table (``undistort_table``) and the Rodrigues matrix (``rodrigues_ref``) are written out here, used by ``restate``,
``calibration`` and ``roundtrip_residual``, and ``check_host_constants`` holds the product's own table and matrix against them.

Tolerances, all derived per case from the two restatements, never from the kernel:
  band_z  = 4 x max |z32 - z64| over the pixels with a finite depth; band_uv = 4 x max(|u32 - u64|, |v32 - v64|) over the pixels with
            a finite depth and z64 > TH - band_z.  (A pixel with z <= TH - band_z is invalid in every evaluation whatever its u, v, and
            a depth of 0 projects through a point a few millimetres from the colour camera, where u, v are of the order 1e9 and
            say nothing: leaving those out makes the band narrower, never wider.)  The factor 4 is this project's usual margin over a
            float32 CPU evaluation: the kernel contracts into FMAs, numpy does not.
  excused = z64 within band_z of TH, or (mask_on_color) u64 or v64 within band_uv of a rounding boundary x.5 (which covers the image
            bounds -0.5 and size - 0.5), or the two restatements disagree on the flag.  At most 2 % of a case's pixels (asserted: a
            condition on the inputs that the restatements alone must meet).  Outside them the device flags equal the float64 flags.
  points  : on pixels valid on the device and in float64, |device - float64| <= 4 x max |p32 - p64| (over the pixels valid in both
            restatements).
  compaction, exact, against the device's own per-pixel output; init_trans within 1 float32 ulp of the float64 mean of the device's
  own valid points (the device sums in double and rounds once); two runs bit-identical.
"""
import functools

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd import depth as D
from lemo_amd.scan import scan_terms

F32, F64 = np.float32, np.float64
EXCUSE_CAP = 0.02
MARGIN = 4.0


def dev(a, device):
    return torch.from_numpy(np.array(a, order='C')).to(device)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ host constants, restated
def rodrigues_ref(r):
    """cv2.Rodrigues for a rotation vector, float64: R = I + sin(t) K + (1 - cos(t)) K K with K the cross-product matrix of r / |r|"""
    r = np.asarray(r, F64)
    t = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if t == 0:
        return np.eye(3)
    a, b, c = r / t
    K = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]], F64)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def undistort_table(camera_mtx, k, H, W):
    """cv2.undistortPoints (no R, no P) for every pixel (u, v) of an H x W image, float64 [H, W, 2]: start at ((u - cx) / fx,
    (v - cy) / fy), then 5 times  x <- (x0 - dx) / cdist, y <- (y0 - dy) / cdist  with  cdist = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
    dx = 2 p1 x y + p2 (r2 + 2 x^2), dy = p1 (r2 + 2 y^2) + 2 p2 x y  and  k = (k1, k2, p1, p2, k3)"""
    fx, fy, cx, cy = camera_mtx[0][0], camera_mtx[1][1], camera_mtx[0][2], camera_mtx[1][2]
    k1, k2, p1, p2, k3 = (float(c) for c in k)
    out = np.empty((H, W, 2), F64)
    x0 = (np.arange(W, dtype=F64) - cx) / fx
    for row in range(H):
        y0 = (F64(row) - cy) / fy
        x, y = x0.copy(), np.full(W, y0)
        for _ in range(5):
            r2 = x * x + y * y
            cdist = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dx) / cdist, (y0 - dy) / cdist
        out[row, :, 0], out[row, :, 1] = x, y
    return out


# ------------------------------------------------------------------------------------------------------------ calibration, scenes
def calibration(H, W, cH, cW):
    """a Kinect-like pair of cameras, intrinsics scaled from 424 x 512 / 1080 x 1920 to the sizes asked for"""
    sx, sy, cx_, cy_ = W / 512.0, H / 424.0, cW / 1920.0, cH / 1080.0
    Rd = rodrigues_ref([0.01, -0.02, 0.005])
    dc = dict(camera_mtx=[[366.0 * sx, 0, 256.7 * sx], [0, 366.0 * sy, 206.3 * sy], [0, 0, 1]], k=[0.0925, -0.2719, 0.0005, -0.0003, 0.0927],
              view_mtx=np.hstack([Rd, [[0.002], [0.001], [-0.003]]]).tolist())
    rc, Tc = [0.003, -0.004, 0.002], [0.052, 0.0005, -0.001]
    cc = dict(camera_mtx=[[1060.5 * cx_, 0, 951.3 * cx_], [0, 1060.4 * cy_, 536.8 * cy_], [0, 0, 1]], k=[0.0519, -0.0563, 0.0008, -0.0006, 0.0134],
              R=rc, T=Tc, view_mtx=np.hstack([rodrigues_ref(rc), np.asarray(Tc)[:, None]]).tolist())
    return dc, cc


# name -> (H, W, B, colour rows, colour columns)
SHAPES = {'5x7': (5, 7, 1, 96, 160), '16x16': (16, 16, 1, 96, 160), '37x300': (37, 300, 3, 96, 160), '64x64': (64, 64, 2, 96, 160),
          'full': (424, 512, 2, 1080, 1920)}
SMALL = ['5x7', '16x16', '37x300', '64x64']


@functools.lru_cache(maxsize=None)
def scene(name, mask_on_color, raw=False):
    """-> dict(depth: what the device gets ([B, H, W] float32, or uint16 with raw), mask uint8).  Frame 0: a wavy surface around 2 m with
    holes and, when the frame is large enough, NaN / +Inf / -Inf pixels; frame 1 (B >= 2): no valid point; frame 2 (B >= 3): no hole and
    an all-zero mask (every pixel valid in the depth-mask branch)."""
    H, W, B, cH, cW = SHAPES[name]
    rng = np.random.default_rng(H * 1000 + W + 7 * mask_on_color)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.empty((B, H, W), F64)
    for b in range(B):
        depth[b] = 2.0 + 0.5 * np.sin(xx * (13.8 / W) + b) + 0.3 * np.cos(yy * (18.4 / H)) + rng.normal(0, 0.01, (H, W))
        if b != 2:
            depth[b][rng.random((H, W)) < 0.1] = 0
    rawv = np.round(depth * 8000).astype(np.uint16)                # the recording's unit: 1 / 8 mm
    depth = ((rawv.astype(F32) * F32(0.125)) * F32(1e-3)).astype(F32)
    if not raw and H * W >= 35:
        depth[0].reshape(-1)[[3, 17, 34]] = [np.nan, np.inf, -np.inf]
    if mask_on_color:
        Y, X = np.mgrid[0:cH, 0:cW]
        mask = np.full((B, cH, cW), 255, np.uint8)
        for b in range(B):
            mask[b][((X - 0.47 * cW - 5 * b) / (0.16 * cW)) ** 2 + ((Y - 0.52 * cH) / (0.39 * cH)) ** 2 < 1] = 0
    else:
        mask = np.zeros((B, H, W), np.uint8)
        for b in range(B):
            mask[b][((xx - 0.5 * W) / (0.3 * W)) ** 2 + ((yy - 0.5 * H) / (0.45 * H)) ** 2 >= 1] = 255
    if B >= 2:
        mask[1] = 255
    if B >= 3:
        mask[2] = 0
    out = dict(depth=rawv if raw else depth, mask=mask)
    for a in out.values():
        a.setflags(write=False)
    return out


def metres(depth, dt, flip=False, depth_scale=1e-3):
    """what the kernel's depth stage computes from its input, in ``dt``"""
    if depth.dtype == np.uint16:
        d = (depth.astype(dt) / dt(8)) * dt(depth_scale)
    else:
        d = depth.astype(dt)
    return d[:, :, ::-1] if flip else d


# ------------------------------------------------------------------------------------------------------------ the restatement
def restate(dt, d, mask, dc, cc, csize, mask_on_color, coord, TH):
    """projection_utils.py:35-90 for B frames in ``dt``; d [B, H, W] metres in ``dt``.  The ray table is float64 for the yardstick and
    the float32-rounded table otherwise.  -> flags bool [B, H, W], pc [B, H, W, 3], u, v [B, H, W] (unrounded; NaN without
    mask_on_color), z"""
    B, H, W = d.shape
    f = lambda a: np.asarray(a, dt)
    rays = undistort_table(dc['camera_mtx'], dc['k'], H, W)
    rays = rays if dt is F64 else rays.astype(F32)
    with np.errstate(all='ignore'):
        if not mask_on_color:
            d = np.where(mask != 0, dt(0), d)
        finite = np.isfinite(d)
        V = f(dc['view_mtx'])
        p = (np.stack([rays[None, ..., 0] * d, rays[None, ..., 1] * d, d], -1) - V[:, 3]) @ V[:, :3]
        Vc = f(cc['view_mtx'])
        pc = p @ Vc[:, :3].T + Vc[:, 3] if coord == 'color' else p
        flags = finite & (pc[..., 2] > dt(TH))
        u = v = np.full(d.shape, np.nan, dt)
        if mask_on_color:
            R, T, k, M = f(rodrigues_ref(cc['R'])), f(cc['T']), f(cc['k']), f(cc['camera_mtx'])
            q = p @ R.T + T
            x, y = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
            r2 = x * x + y * y
            cd = dt(1) + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
            xd = x * cd + dt(2) * k[2] * x * y + k[3] * (r2 + dt(2) * x * x)
            yd = y * cd + k[2] * (r2 + dt(2) * y * y) + dt(2) * k[3] * x * y
            u, v = M[0, 0] * xd + M[0, 2], M[1, 1] * yd + M[1, 2]
            ui, vi = np.round(u), np.round(v)
            inside = (ui >= 0) & (ui < csize[1]) & (vi >= 0) & (vi < csize[0])
            bi = np.broadcast_to(np.arange(B)[:, None, None], d.shape)
            keep = np.zeros(d.shape, bool)
            keep[inside] = mask[bi[inside], vi[inside].astype(np.int64), ui[inside].astype(np.int64)] == 0
            flags = flags & keep
    return flags, pc, u, v, pc[..., 2], finite


def roundtrip_residual(dc, H, W):
    """project(undistort(pixel)) - pixel for the IR camera in float64: largest absolute residual in pixels"""
    r = undistort_table(dc['camera_mtx'], dc['k'], H, W)
    x, y, k, M = r[..., 0], r[..., 1], np.asarray(dc['k'], F64), np.asarray(dc['camera_mtx'], F64)
    r2 = x * x + y * y
    cd = 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    v, u = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing='ij')
    return float(max(np.abs(M[0, 0] * xd + M[0, 2] - u).max(), np.abs(M[1, 1] * yd + M[1, 2] - v).max()))


@functools.lru_cache(maxsize=None)
def reference(name, mask_on_color, coord, raw=False, flip=False, TH=1e-2):
    """the two restatements of a case and everything derived from them; computed once, shared, read-only"""
    H, W, B, cH, cW = SHAPES[name]
    dc, cc = calibration(H, W, cH, cW)
    sc = scene(name, mask_on_color, raw)
    f64, p64, u64, v64, z64, fin = restate(F64, metres(sc['depth'], F64, flip), sc['mask'], dc, cc, (cH, cW), mask_on_color, coord, TH)
    f32, p32, u32, v32, z32, _ = restate(F32, metres(sc['depth'], F32, flip), sc['mask'], dc, cc, (cH, cW), mask_on_color, coord, TH)
    with np.errstate(all='ignore'):
        band_z = MARGIN * float(np.abs(z32.astype(F64) - z64)[fin].max()) if fin.any() else 0.0
        excused = (np.abs(z64 - TH) < band_z) | (f32 != f64)
        band_uv = 0.0
        if mask_on_color:
            cand = fin & (z64 > TH - band_z)
            if cand.any():
                band_uv = MARGIN * float(max(np.abs(u32.astype(F64) - u64)[cand].max(), np.abs(v32.astype(F64) - v64)[cand].max()))
            near = lambda a: np.abs(a - np.floor(a) - 0.5) < band_uv
            excused |= cand & (near(u64) | near(v64))
        both = f64 & f32
        perr = float(np.abs(p32.astype(F64) - p64)[both].max()) if both.any() else 0.0
    out = dict(flags=f64, points=p64, u=u64, v=v64, excused=excused, band_z=band_z, band_uv=band_uv, perr=perr, disagree=int((f32 != f64).sum()))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def projection(lib, device, name):
    H, W, B, cH, cW = SHAPES[name]
    dc, cc = calibration(H, W, cH, cW)
    return D.DepthProjection(depth_cam=dc, color_cam=cc, color_size=(cH, cW), device=device, _lib=lib)


def run(lib, device, name, mask_on_color, coord, S, raw=False, flip=False, TH=1e-2, proj=None):
    """one create_scan with per-pixel outputs into a NaN-filled scan -> dict of numpy arrays"""
    H, W, B, cH, cW = SHAPES[name]
    sc = scene(name, mask_on_color, raw)
    proj = proj or projection(lib, device, name)
    out = torch.full((B, S, 3), float('nan'), dtype=torch.float32, device=device)
    res = proj.create_scan(dev(sc['mask'], device), dev(sc['depth'], device), mask_on_color=mask_on_color, coord=coord, TH=TH, S=S, raw=raw,
                           flip=flip, return_pixels=True, out=out)
    assert res['scan'] is out
    assert res['scan'].dtype == torch.float32 and res['scan_point_num'].dtype == torch.int32 and res['n_valid'].dtype == torch.int32
    assert res['init_trans'].shape == (B, 3) and res['points'].shape == (B, H, W, 3) and res['valid'].dtype == torch.uint8
    return {k: host(v) for k, v in res.items()}


# ------------------------------------------------------------------------------------------------------------ checks
def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_host_constants(lib, device, name):
    """the product's ray table and colour rotation against this module's own restatements.  The table on the device is a float64
    table rounded to float32 once: it may differ from the restated one by that rounding (half a float32 ulp) plus the few float64
    ulps by which two float64 evaluations in another operation order differ (1e-13 of a value of order 1 is 450 of them)."""
    H, W, B, cH, cW = SHAPES[name]
    dc, cc = calibration(H, W, cH, cW)
    R = rodrigues_ref(cc['R'])
    t = float(np.linalg.norm(cc['R']))
    axis = np.asarray(cc['R'], F64) / t
    # the restatement itself: a rotation about the vector by its length, right-handed
    assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -52 and abs(np.linalg.det(R) - 1) <= 8 * 2.0 ** -52
    assert np.abs(R @ axis - axis).max() <= 8 * 2.0 ** -52 and abs(np.trace(R) - (1 + 2 * np.cos(t))) <= 8 * 2.0 ** -52
    assert np.abs((R - R.T) / 2 - np.sin(t) * np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])).max() <= 8 * 2.0 ** -52
    proj = projection(lib, device, name)
    err_R = float(np.abs(proj.Rc - R).max())
    table = undistort_table(dc['camera_mtx'], dc['k'], H, W)
    rays = host(proj.rays(H, W))
    assert rays.dtype == F32 and rays.shape == (H, W, 2)
    bound = 0.5 * np.spacing(np.abs(table).astype(F32)).astype(F64) + 1e-13
    err_t = np.abs(rays.astype(F64) - table)
    print(f'{name}: Rc vs restated Rodrigues {err_R:.2e} (bound {8 * 2.0 ** -52:.2e}); ray table vs restated undistortion: worst '
          f'{float(err_t.max()):.3e}, worst error / bound {float((err_t / bound).max()):.3f}')
    assert err_R <= 8 * 2.0 ** -52
    assert np.all(err_t <= bound)
    cal, _ = proj._calibration(H, W)
    assert np.abs(np.array(cal.Rc[:], F64) - R.reshape(-1)).max() <= 2.0 ** -25 + 1e-13      # entries <= 1: half a float32 ulp
    assert np.array_equal(np.array(cal.view_d[:], F32), np.asarray(dc['view_mtx'], F32).reshape(-1))
    assert np.array_equal(np.array(cal.view_c[:], F32), np.asarray(cc['view_mtx'], F32).reshape(-1))
    assert np.array_equal(np.array(cal.k[:], F32), np.asarray(cc['k'], F32)) and np.array_equal(np.array(cal.Tc[:], F32), np.asarray(cc['T'], F32))
    M = np.asarray(cc['camera_mtx'], F32)
    assert (cal.fx, cal.fy, cal.cx, cal.cy) == (M[0, 0], M[1, 1], M[0, 2], M[1, 2]) and (cal.cH, cal.cW) == (cH, cW)


def check_compaction(r, S):
    """exact, against the device's own per-pixel output"""
    B = r['scan'].shape[0]
    valid = r['valid'].astype(bool)
    assert set(np.unique(r['valid'])) <= {0, 1}
    for b in range(B):
        pts = r['points'][b][valid[b]]                             # row-major
        n = len(pts)
        assert int(r['n_valid'][b]) == n and int(r['scan_point_num'][b]) == min(n, S), (b, n, r['n_valid'][b], r['scan_point_num'][b])
        assert same_bits(r['scan'][b, :min(n, S)], pts[:S]), f'frame {b}: the scan is not the first points in row-major order'
        pad = r['scan'][b, min(n, S):]
        assert np.all(pad == 0.0) and not np.isnan(pad).any(), f'frame {b}: the pad is not written as zeros'
        it = r['init_trans'][b]
        if n == 0:
            assert np.isnan(it).all()
        else:
            mean = pts.astype(F64).mean(0)
            assert np.all(np.abs(it.astype(F64) - mean) <= np.spacing(np.abs(mean).astype(F32)).astype(F64)), (b, it, mean)


def check_against_float64(r, ref, label):
    B = r['valid'].shape[0]
    valid = r['valid'].astype(bool)
    npx = valid[0].size
    share = ref['excused'].reshape(B, -1).mean(1)
    print(f'{label}: valid {valid.reshape(B, -1).sum(1)}, float64 {ref["flags"].reshape(B, -1).sum(1)}, excused share {share} (cap {EXCUSE_CAP}), '
          f'restatements disagree on {ref["disagree"]} of {B * npx}, band uv {ref["band_uv"]:.3e} px, band z {ref["band_z"]:.3e} m')
    assert ref['excused'].mean() <= EXCUSE_CAP, f'{label}: {ref["excused"].mean()} of the pixels are excused'
    bad = (valid != ref['flags']) & ~ref['excused']
    assert not bad.any(), f'{label}: {bad.sum()} flags differ from float64 outside the excused pixels'
    both = valid & ref['flags']
    err = float(np.abs(r['points'][both].astype(F64) - ref['points'][both]).max()) if both.any() else 0.0
    print(f'{label}: points: device vs float64 {err:.3e} m, float32 restatement vs float64 {ref["perr"]:.3e} m (bound {MARGIN} x)')
    assert err <= MARGIN * ref['perr']


def check_case(lib, device, name, mask_on_color, coord):
    """flags and points against float64; compaction at S below, equal to and above the count; special frames; repeatability"""
    H, W, B, cH, cW = SHAPES[name]
    ref = reference(name, mask_on_color, coord)
    proj = projection(lib, device, name)
    label = f'{name} mask_on_color={mask_on_color} coord={coord}'
    print(f'{label}: project(undistort(pixel)) - pixel: {roundtrip_residual(calibration(H, W, cH, cW)[0], H, W):.3e} px (not gated)')
    S0 = 20000 if name == 'full' else H * W + 50                 # the loader's S at full size (it truncates there); else: padding
    r = run(lib, device, name, mask_on_color, coord, S0, proj=proj)
    check_against_float64(r, ref, label)
    check_compaction(r, S0)
    again = run(lib, device, name, mask_on_color, coord, S0, proj=proj)
    assert all(same_bits(r[k], again[k]) for k in r), 'two runs differ'
    n0 = int(r['n_valid'][0])
    assert n0 > 0, 'frame 0 must have valid points'
    if B >= 2:
        assert int(r['n_valid'][1]) == 0 and np.isnan(r['init_trans'][1]).all() and np.all(r['scan'][1] == 0.0)
    if B >= 3 and not mask_on_color:
        assert int(r['n_valid'][2]) == H * W, 'every pixel of frame 2 is valid in the depth-mask branch'
    if name == 'full':
        assert n0 > S0, 'the full-size case must truncate'
        return
    assert n0 < S0
    sizes = {n0, max(1, n0 - 1), max(1, n0 // 2 + 1)}             # equal to the count; truncation inside a wave and inside a group
    if n0 > 70:
        sizes |= {n0 - 37, 67}
    for S in sorted(sizes):
        rs = run(lib, device, name, mask_on_color, coord, S, proj=proj)
        assert same_bits(rs['points'], r['points']) and same_bits(rs['valid'], r['valid']) and same_bits(rs['init_trans'], r['init_trans'])
        check_compaction(rs, S)


def check_raw(lib, device, flip):
    """uint16 input (with and without flip) against float64, and against the float path on the pre-flipped, pre-scaled image"""
    name, mask_on_color, coord = '37x300', True, 'color'
    H, W, B, cH, cW = SHAPES[name]
    ref = reference(name, mask_on_color, coord, raw=True, flip=flip)
    proj = projection(lib, device, name)
    S = H * W
    r = run(lib, device, name, mask_on_color, coord, S, raw=True, flip=flip, proj=proj)
    check_against_float64(r, ref, f'raw flip={flip}')
    check_compaction(r, S)
    sc = scene(name, mask_on_color, True)
    pre = np.ascontiguousarray(metres(sc['depth'], F32, flip))
    res = proj.create_scan(dev(sc['mask'], device), dev(pre, device), mask_on_color=mask_on_color, coord=coord, S=S, return_pixels=True)
    assert np.array_equal(host(res['valid']), r['valid']), 'flags differ between the raw and the float path'
    both = r['valid'].astype(bool)
    err = float(np.abs(host(res['points']).astype(F64) - r['points'].astype(F64))[both].max())
    print(f'raw flip={flip}: raw path vs float path {err:.3e} m (bound {MARGIN * ref["perr"]:.3e})')
    assert err <= MARGIN * ref['perr']
    assert int(r['n_valid'][0]) > 0


def check_round_trip(lib, device):
    """create_scan's output goes straight into scan_terms, which accepts the counts"""
    name = '37x300'
    H, W, B, cH, cW = SHAPES[name]
    sc = scene(name, True)
    proj = projection(lib, device, name)
    out = proj.create_scan(dev(sc['mask'], device), dev(sc['depth'], device), S=500)
    assert int(out['n_valid'][0]) > 500 and int(out['scan_point_num'][0]) == 500       # more survivors than S: the capped count goes on
    rng = np.random.default_rng(3)
    centre = host(out['init_trans'])[0]
    verts = np.stack([centre + rng.normal(0, 0.2, (12, 3)) for _ in range(B)]).astype(F32)
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7, 8], [8, 9, 10], [10, 11, 0]], np.int64)
    mask = dev(np.arange(12) % 3 != 0, device)
    s2m, m2s = scan_terms(dev(verts, device), faces, out['scan'], out['scan_point_num'], mask, 1.0, 1.0, _lib=lib)
    print(f'round trip: s2m {float(s2m):.6f}, m2s {float(m2s):.6f}')
    assert np.isfinite(float(s2m)) and np.isfinite(float(m2s)) and float(s2m) > 0 and float(m2s) > 0


def check_drop_in(lib, device):
    """the reference-named Projection (numpy, one frame) against the batched call"""
    name = '64x64'
    H, W, B, cH, cW = SHAPES[name]
    dc, cc = calibration(H, W, cH, cW)
    drop = D.Projection(depth_cam=dc, color_cam=cc, color_size=(cH, cW), device=device, _lib=lib)
    for mask_on_color in (True, False):
        sc = scene(name, mask_on_color)
        for coord in ('color', None):
            r = run(lib, device, name, mask_on_color, coord, H * W)
            depth_im = sc['depth'][0].astype(F64)
            keep = depth_im.copy()
            got = drop.create_scan(sc['mask'][0], depth_im, mask_on_color=mask_on_color, coord=coord)
            assert same_bits(depth_im, keep), 'the drop-in must not modify the depth image'
            n = int(r['n_valid'][0])
            assert set(got) == {'points', 'colors'} and got['points'].dtype == F64 and got['points'].shape == (n, 3)
            assert np.array_equal(got['points'], r['scan'][0, :n].astype(F64))
            assert got['colors'].shape == (n, 3) and np.all(got['colors'] == np.array([1.00, 0.75, 0.80]))
    with pytest.raises(NotImplementedError):
        drop.create_scan(sc['mask'][0], sc['depth'][0], color_im=np.zeros((cH, cW, 3)))
    assert drop.create_scan(sc['mask'][0], np.zeros((0, W))) == {'v': []}        # projection_utils.py:57-58
    # unproject_depth_image: the per-pixel points of coord=None, bit for bit; projectPoints against float64
    sc = scene(name, True)
    r = run(lib, device, name, True, None, H * W)
    pts = drop.unproject_depth_image(sc['depth'][0], drop.depth_cam)
    assert pts.shape == (H, W, 3) and np.array_equal(pts.astype(F32), r['points'][0], equal_nan=True)
    ref = reference(name, True, None)
    sel = r['valid'][0].astype(bool) & ref['flags'][0]
    uv = drop.projectPoints(r['points'][0][sel], drop.color_cam)
    err = float(max(np.abs(uv[:, 0] - ref['u'][0][sel]).max(), np.abs(uv[:, 1] - ref['v'][0][sel]).max()))
    print(f'projectPoints vs float64: {err:.3e} px (bound {ref["band_uv"]:.3e})')
    assert uv.shape == (int(sel.sum()), 2) and err <= ref['band_uv']


def check_refusals(lib, device, monkeypatch):
    """every ValueError / NotImplementedError path raises before a launch"""
    launched = []
    for fn in ('depth_scan', 'depth_unproject'):
        monkeypatch.setattr(lib, fn, lambda *a, _n=fn: launched.append(_n) or 0)
    name = '16x16'
    H, W, B, cH, cW = SHAPES[name]
    dc, cc = calibration(H, W, cH, cW)
    proj = projection(lib, device, name)
    sc = scene(name, True)
    d, m = dev(sc['depth'], device), dev(sc['mask'], device)
    md = dev(scene(name, False)['mask'], device)
    raw = dev(scene(name, True, True)['depth'], device)
    E = ValueError                                                # every refusal, a tensor on the wrong device included
    bad = [dict(depth=d.double()), dict(depth=d[0]), dict(depth=host(d)), dict(depth=raw), dict(depth=d, raw=True), dict(depth=d[:, :0]),
           dict(mask=md), dict(mask=m.float()), dict(mask=m[:, :-1]), dict(mask=host(m)), dict(mask=m, mask_on_color=False),
           dict(mask=torch.cat([m, m])), dict(S=0), dict(S=(1 << 20) + 1), dict(coord='depth'), dict(TH=float('nan')), dict(depth_scale=float('inf')),
           dict(out=torch.empty(B, 7, 3, device=device), S=8), dict(out=torch.empty(B, 8, 3, dtype=torch.float64, device=device), S=8),
           dict(depth=torch.zeros(1025, 2, 2, device=device), mask=torch.zeros(1025, cH, cW, dtype=torch.uint8, device=device)),
           dict(depth=torch.zeros(1, 2049, 2048, device=device), mask=torch.zeros(1, cH, cW, dtype=torch.uint8, device=device))]
    for kw in bad:
        args = dict(mask=m, depth=d)
        args.update(kw)
        with pytest.raises(E):
            proj.create_scan(**args)
    for kw in (dict(depth=d.double()), dict(depth=d[0]), dict(depth=raw), dict(depth=d, depth_scale=float('nan'))):
        with pytest.raises(E):
            proj.unproject_depth_image(**kw)
    for kw in (dict(points=d), dict(points=d.double()[..., :3]), dict(points=torch.zeros(4, 3, device=device), cam='ir')):
        with pytest.raises(E):
            proj.project_points(**kw)
    if device.type != 'cpu':
        with pytest.raises(E):
            proj.create_scan(m.cpu(), d)
        with pytest.raises(E):
            proj.create_scan(m, d.cpu())
    for kw in (dict(), dict(depth_cam=dc), dict(depth_cam=dc, color_cam={k: v for k, v in cc.items() if k != 'R'}),
               dict(depth_cam=dc, color_cam=cc, color_size=(0, 10)), dict(depth_cam=dict(dc, k=[0.0] * 4), color_cam=cc)):
        with pytest.raises(ValueError):
            D.DepthProjection(device=device, _lib=lib, **kw)
    drop = D.Projection(depth_cam=dc, color_cam=cc, color_size=(cH, cW), device=device, _lib=lib)
    with pytest.raises(NotImplementedError):
        drop.create_scan(sc['mask'][0], sc['depth'][0], color_im=np.zeros((cH, cW, 3)), mask_on_color=True)
    with pytest.raises(ValueError):
        drop.create_scan(sc['mask'], sc['depth'], mask_on_color=True)          # a batch: the drop-in takes one frame
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    cal, _ = proj._calibration(H, W)
    import ctypes as C

    def ds(B=1, H=2, W=2, S=4, depth=1, mask=1, raw=0, flip=0, moc=1, cc_=1, TH=0.01, scale=1e-3, c=cal, ws=1, wsb=1 << 30, pts=None, val=None):
        return lib.depth_scan(depth, raw, flip, scale, mask, moc, cc_, TH, C.byref(c) if c is not None else None, B, H, W, S, 1, 1, 1, 1, pts, val,
                              ws, wsb, None)
    assert ds(B=0) == 10001 and ds(B=1025) == 10001 and ds(H=0) == 10001 and ds(H=2049, W=2048) == 10001 and ds(S=0) == 10001
    assert ds(S=(1 << 20) + 1) == 10001
    assert ds(depth=None) == 10002 and ds(mask=None) == 10002 and ds(c=None) == 10002 and ds(raw=2) == 10002 and ds(moc=-1) == 10002
    assert ds(TH=float('nan')) == 10002 and ds(scale=float('inf')) == 10002 and ds(ws=None) == 10002 and ds(wsb=31) == 10002 and ds(pts=1) == 10002
    empty = _hip.DepthCalib()
    assert ds(c=empty) == 10002                                   # no ray table
    small = _hip.DepthCalib.from_buffer_copy(cal)
    small.cW = 0
    assert ds(c=small) == 10001
    un = lambda B=1, H=2, W=2, depth=1, pts=1, c=cal: lib.depth_unproject(depth, 0, 0, 1e-3, C.byref(c), B, H, W, pts, None)
    assert un(B=0) == 10001 and un(W=0) == 10001 and un(depth=None) == 10002 and un(pts=None) == 10002 and un(c=empty) == 10002
    assert lib.depth_scan_ws_bytes(0, 2, 2) == -1 and lib.depth_scan_ws_bytes(1, 2049, 2048) == -1
    assert lib.depth_scan_ws_bytes(2, 424, 512) == 2 * 848 * 32 and lib.depth_scan_ws_bytes(3, 5, 7) == 3 * 32
