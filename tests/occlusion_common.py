"""The cases of the occlusion-mask tests (lemo_amd.occlusion, csrc/occlusion_kernels.hip), shared by the emulator suite
(tests/test_occlusion_emu.py) and the GPU suite (tests/test_occlusion_gpu.py).  Every figure is printed before it is asserted.

THE YARDSTICK IS NOT PYRENDER.  The reference's utils/get_occlusion_mask.py renders with pyrender, which is not installed where
this project is built, so no fixture could be generated from it.  The yardstick is a float64 numpy restatement of the geometry the
module documents: pinhole u = fx X / Z + cx, v = fy Y / Z + cy (camera space y down, z forward), pixel [y][x] sampling the ray
through (x + 0.5, y + 0.5), coverage by the sign of the three homogeneous edge functions, depth = ray-plane Z of the nearest hit with
znear <= Z <= zfar (0 = no hit), back faces culled iff ((v1 - v0) x (v2 - v0)) . v0 >= 0, points projected with their own
intrinsics and truncated toward zero, and the rule of get_occlusion_mask.py:197-200.  What it says about pyrender (pixel centres,
culling) rests on reading, not on a run.

Excused from exact comparison ("ambiguous") are: pixels whose centre is within 1e-3 px of an edge of any triangle whose
bounding box contains it; queries whose projected u or v is within 1e-3 of an integer; queries with |depth_body - depth_scene -
thresh| < 1e-4 m; queries on a pixel that is ambiguous in the scene depth.  At most 0.5 % of a depth map and 2 % of a mask may be
excused, and a plain float32 numpy evaluation of the same restatement has to stay inside those caps too (asserted).  Everything else
matches exactly -- coverage and mask bit -- and depths agree with float64 within 4 x the largest error of the float32 evaluation on
the same inputs (the error of the arithmetic, not of the kernel; 4 for a different order of operations).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd.occlusion import OcclusionMasker, SceneDepth, render_depth

EDGE_PX, INT_PX, THRESH_M = 1e-3, 1e-3, 1e-4
CAP_PIXELS, CAP_QUERIES = 0.005, 0.02
NOPIX = -2 ** 31
F32, F64 = np.float32, np.float64


def camera(W, H, cull=True, full=False):
    """intrinsics as the float32 values the C ABI carries; small images get a 64-pixel-wide version of PROX's camera"""
    if full:
        c = dict(W=1920, H=1080, fx=1060.53, fy=1060.38, cx=951.30, cy=536.77)
    else:
        c = dict(W=W, H=H, fx=60.53, fy=60.38, cx=W / 2 - 0.7, cy=H / 2 + 0.27)
    c.update(znear=0.05, zfar=100.0)
    c = {k: (v if k in 'WH' else float(F32(v))) for k, v in c.items()}
    c['cull_backface'] = bool(cull)
    return c


def proj_of(cam):
    """the points' own intrinsics: fx = fy like get_occlusion_mask.py:132-134 (the render's fy differs)"""
    return float(F32(cam['fx'])), float(F32(cam['fx']))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _setup(verts, faces, xf, cam, dt):
    """per-triangle constants in dtype dt: edge vectors E [F, 3, 3], normal n, D = n . p0, draw flag, bounding box"""
    v = np.asarray(verts, F32).astype(dt)
    if xf is not None:
        m = np.asarray(xf, F32).astype(dt)
        v = np.stack([((m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2]) + m[k, 3] for k in range(3)], -1)
    f = np.asarray(faces, np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    E = np.stack([_cross(p1, p2 - p1), _cross(p2, p0 - p2), _cross(p0, p1 - p0)], 1)
    n = _cross(p1 - p0, p2 - p0)
    D = (n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2]
    z = np.stack([p0[:, 2], p1[:, 2], p2[:, 2]], -1)
    zmin, zmax = z.min(-1), z.max(-1)
    znear, zfar = dt(cam['znear']), dt(cam['zfar'])
    fin = np.isfinite(np.concatenate([p0, p1, p2], -1)).all(-1)
    live = fin & ~((zmax < znear) | (zmin > zfar))
    front = zmin >= znear
    W, H = cam['W'], cam['H']
    with np.errstate(all='ignore'):
        X = np.stack([p0[:, 0], p1[:, 0], p2[:, 0]], -1)
        Y = np.stack([p0[:, 1], p1[:, 1], p2[:, 1]], -1)
        u = (dt(cam['fx']) * X) / z + dt(cam['cx'])
        w = (dt(cam['fy']) * Y) / z + dt(cam['cy'])
        span = lambda lo, hi, n_: (np.clip(np.floor(lo) - 1, 0, n_), np.clip(np.floor(hi) + 1, -1, n_ - 1))
        x0, x1 = span(u.min(-1), u.max(-1), W)
        y0, y1 = span(w.min(-1), w.max(-1), H)
    x0, x1 = np.where(front, x0, 0), np.where(front, x1, W - 1)
    y0, y1 = np.where(front, y0, 0), np.where(front, y1, H - 1)
    box = np.nan_to_num(np.stack([x0, x1, y0, y1], -1)).astype(np.int64)
    live &= (box[:, 0] <= box[:, 1]) & (box[:, 2] <= box[:, 3])
    draw = live & ((D < 0) if cam['cull_backface'] else True)
    return dict(E=E, n=n, D=D, live=live, draw=draw, box=box)


def _rays(x, y, cam, dt):
    dx = ((np.asarray(x).astype(dt) + dt(0.5)) - dt(cam['cx'])) / dt(cam['fx'])
    dy = ((np.asarray(y).astype(dt) + dt(0.5)) - dt(cam['cy'])) / dt(cam['fy'])
    return dx, dy


def _hits(S, idx, dx, dy, cam, dt, want_edge):
    """triangles idx (array or scalar) against rays (dx, dy), broadcast -> Z (inf without a hit), near-an-edge flag"""
    E, n, D = S['E'][idx], S['n'][idx], S['D'][idx]
    ex = lambda a: a[..., None] if np.ndim(idx) else a        # [F'] -> [F', 1] against rays [N]
    e = [(ex(E[..., i, 0]) * dx + ex(E[..., i, 1]) * dy) + ex(E[..., i, 2]) for i in range(3)]
    inside = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
    nd = (ex(n[..., 0]) * dx + ex(n[..., 1]) * dy) + ex(n[..., 2])
    with np.errstate(all='ignore'):
        Z = ex(D) / nd
        hit = inside & (Z >= dt(cam['znear'])) & (Z <= dt(cam['zfar']))
        near = None
        if want_edge:
            # distance in pixels to the LINE of edge i: |e_i| over the gradient of e_i per pixel (a degenerate edge, 0 / 0, counts as
            # near).  Near the edge itself: near its line, and beside the segment (the other two edge functions agree in sign) or
            # at one of its ends (near another edge's line as well).
            line = [~(np.abs(e[i]) / np.hypot(ex(E[..., i, 0]) / cam['fx'], ex(E[..., i, 1]) / cam['fy']) >= EDGE_PX) for i in range(3)]
            near = np.zeros(np.broadcast(e[0], dx).shape, bool)
            for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                near |= line[i] & ((e[j] * e[k] >= 0) | line[j] | line[k])
    return np.where(hit, Z, np.inf), near


def restate_raster(verts, faces, xf, cam, dt=F64, want_amb=True):
    """brute force over all triangles -> depth [H, W] (dt, 0 = no hit), ambiguous [H, W]"""
    S = _setup(verts, faces, xf, cam, dt)
    depth = np.full((cam['H'], cam['W']), np.inf, dt)
    amb = np.zeros((cam['H'], cam['W']), bool)
    for f in np.nonzero(S['live'])[0]:
        x0, x1, y0, y1 = S['box'][f]
        dx, dy = _rays(np.arange(x0, x1 + 1)[None, :], np.arange(y0, y1 + 1)[:, None], cam, dt)
        Z, near = _hits(S, int(f), dx, dy, cam, dt, want_amb)
        if S['draw'][f]:
            sub = depth[y0:y1 + 1, x0:x1 + 1]
            np.minimum(sub, Z, out=sub)
        if want_amb:
            amb[y0:y1 + 1, x0:x1 + 1] |= near
    return np.where(np.isfinite(depth), depth, 0).astype(dt), amb


def restate_at(verts, faces, xf, cam, px, py, dt=F64, want_amb=True, chunk=4096):
    """the same at a list of pixels only -> depth [N], ambiguous [N]"""
    S = _setup(verts, faces, xf, cam, dt)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    dx, dy = _rays(px, py, cam, dt)
    depth, amb = np.full(len(px), np.inf, dt), np.zeros(len(px), bool)
    live = np.nonzero(S['live'])[0]
    for lo in range(0, len(live), chunk):
        idx = live[lo:lo + chunk]
        b = S['box'][idx]
        inbox = (px >= b[:, 0:1]) & (px <= b[:, 1:2]) & (py >= b[:, 2:3]) & (py <= b[:, 3:4])
        Z, near = _hits(S, idx, dx, dy, cam, dt, want_amb)
        Z = np.where(inbox & S['draw'][idx][:, None], Z, np.inf)
        depth = np.minimum(depth, Z.min(0))
        if want_amb:
            amb |= (near & inbox).any(0)
    return np.where(np.isfinite(depth), depth, 0).astype(dt), amb


def project(points, cam, pfx, pfy, dt):
    """PerspectiveCamera.forward + astype(int) -> u, v (dt), pixel x, y (NOPIX where not finite), in-image flag"""
    p = np.asarray(points, F32).astype(dt)
    with np.errstate(all='ignore'):
        u = dt(pfx) * (p[..., 0] / p[..., 2]) + dt(cam['cx'])
        v = dt(pfy) * (p[..., 1] / p[..., 2]) + dt(cam['cy'])
        ok = (np.abs(u) < 2147483520.0) & (np.abs(v) < 2147483520.0)
    x = np.where(ok, np.trunc(np.where(ok, u, 0)), NOPIX).astype(np.int64)
    y = np.where(ok, np.trunc(np.where(ok, v, 0)), NOPIX).astype(np.int64)
    inimg = ok & (x >= 0) & (x < cam['W']) & (y >= 0) & (y < cam['H'])
    return u, v, x, y, inimg


def restate_query(verts, faces, points, cam, body_cull, pfx, pfy, scene_at, thresh, dt=F64):
    """verts [T, V, 3], points [T, P, 3]; scene_at(px, py) -> (depth, ambiguous) of the scene at pixels.
    -> dict(mask, depth_body, x, y, inimg, amb), each [T, P]"""
    T, P = points.shape[:2]
    u, v, x, y, inimg = project(points, cam, pfx, pfy, dt)
    bcam = dict(cam, cull_backface=body_cull)
    db, amb = np.zeros((T, P), dt), np.zeros((T, P), bool)
    for t in range(T):
        sel = np.nonzero(inimg[t])[0]
        if len(sel):
            db[t, sel], amb[t, sel] = restate_at(verts[t], faces, None, bcam, x[t, sel], y[t, sel], dt, want_amb=dt is F64)
    ds, samb = np.zeros((T, P), dt), np.zeros((T, P), bool)
    if inimg.any():
        ds[inimg], samb[inimg] = scene_at(x[inimg], y[inimg])
    diff = db - ds
    occluded = inimg & (ds != 0) & (diff > dt(thresh))
    with np.errstate(all='ignore'):
        near_int = np.isfinite(u) & np.isfinite(v) & ((np.abs(u - np.round(u)) < INT_PX) | (np.abs(v - np.round(v)) < INT_PX))
    amb = amb | samb | near_int | (inimg & (ds != 0) & (np.abs(diff - thresh) < THRESH_M))
    return dict(mask=(~occluded).astype(F32), depth_body=db, x=x, y=y, inimg=inimg, amb=amb)


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def _backproject(u, v, z, cam):
    return np.stack([z * (u - cam['cx']) / cam['fx'], z * (v - cam['cy']) / cam['fy'], z], -1)


def random_triangles(F, seed, cam, radius_px=6.0, zlo=1.5, zhi=5.0):
    """F triangles in front of the camera, half of each winding, across (and a little beyond) the image; some bounding boxes are
    above the kernel's big-triangle threshold of 256 pixels, most below"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(zlo, zhi, F)
    c = _backproject(rng.uniform(-6, cam['W'] + 6, F), rng.uniform(-6, cam['H'] + 6, F), z, cam)
    r = (z * radius_px / cam['fx'])[:, None, None] * rng.uniform(0.3, 1.0, (F, 1, 1))
    verts = (c[:, None, :] + rng.standard_normal((F, 3, 3)) * r).reshape(-1, 3).astype(F32)
    return verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def face_camera(verts, faces):
    """every triangle wound counter-clockwise as the camera at the origin sees it (so that culling keeps it)"""
    v = verts.astype(F64)
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    D = (np.cross(p1 - p0, p2 - p0) * p0).sum(-1)
    out = faces.copy()
    out[D > 0] = out[D > 0][:, [0, 2, 1]]
    return out


def fullscreen_pair(cam, z=(4.0, 4.6, 5.2, 4.3)):
    """two triangles that cover every pixel (a non-planar quad reaching past the image), facing the camera"""
    W, H = cam['W'], cam['H']
    q = np.stack([_backproject(-0.013 * W - 9.3, -0.02 * H - 7.1, z[0], cam), _backproject(1.017 * W + 11.7, -0.015 * H - 8.4, z[1], cam),
                  _backproject(1.021 * W + 12.9, 1.03 * H + 9.6, z[2], cam), _backproject(-0.011 * W - 10.2, 1.025 * H + 6.8, z[3], cam)])
    return q.astype(F32), face_camera(q.astype(F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def near_crossers(cam):
    """triangles that cross the near plane and reach behind the camera, of both windings, plus one that lies wholly behind it"""
    W, H = cam['W'], cam['H']
    P = lambda u, v, z: _backproject(u, v, z, cam)
    tris = [[P(0.2 * W, 0.3 * H, 2.0), P(0.7 * W, 0.25 * H, 2.5), np.array([0.31, 0.22, -1.0])],
            [P(0.8 * W, 0.9 * H, 3.0), np.array([-0.4, 0.35, -0.5]), P(0.3 * W, 0.8 * H, 1.2)],
            [P(0.5 * W, 0.5 * H, 0.02), P(0.9 * W, 0.4 * H, 1.0), P(0.6 * W, 0.95 * H, 0.8)],
            [np.array([0.1, 0.2, -2.0]), np.array([0.5, -0.3, -1.0]), np.array([-0.4, 0.1, -3.0])]]
    v = np.asarray(tris, F64).reshape(-1, 3).astype(F32)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + off); off += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int32)


def rigid(seed):
    """a cam2world that is no identity: rotation by 0.4 rad about a random axis, translation of about a metre"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(3); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.4) * K + (1 - np.cos(0.4)) * K @ K
    m = np.eye(4); m[:3, :3] = R; m[:3, 3] = rng.uniform(-1, 1, 3)
    return m


RASTER_MESHES = ('F1', 'F63', 'F65', 'F300', 'full', 'near')
RASTER_SIZES = ((64, 48), (67, 45))


@functools.lru_cache(maxsize=None)
def raster_case(name, W, H, cull, moved, full=False):
    """(verts as handed to the raster, faces, cam2world or None, cam, depth64, ambiguous, depth32), computed once"""
    cam = camera(W, H, cull, full)
    if name.startswith('F'):
        mesh = random_triangles(int(name[1:]), 100 + int(name[1:]) + W, cam)
    elif name == 'full':
        mesh = join(fullscreen_pair(cam), random_triangles(20, 7 + W, cam, zlo=1.5, zhi=3.5))
    elif name == 'near':
        mesh = join(near_crossers(cam), random_triangles(12, 9 + W, cam))
    elif name == 'hd':                                       # GPU only: about 5000 triangles at 1920 x 1080 with the two full-screen ones
        mesh = join(fullscreen_pair(cam), random_triangles(5000, 11, cam, radius_px=14.0, zlo=1.5, zhi=3.9))
    verts, faces = mesh
    c2w = xf = None
    if moved:                                                # the mesh in world coordinates; the raster undoes it with inv(cam2world)
        c2w = rigid(5)
        verts = (verts.astype(F64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)
        xf = np.linalg.inv(c2w)[:3].astype(F32)
    d64, amb = restate_raster(verts, faces, xf, cam, F64)
    d32, _ = restate_raster(verts, faces, xf, cam, F32, want_amb=False)
    return verts, faces, c2w, cam, d64, amb, d32


def dev(a, device, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def compare_depth(got, d64, amb, d32, what):
    """coverage exact and depth within 4 x the float32 restatement's own error, outside the excused pixels; the caps"""
    cov64, cov32, covg = d64 != 0, d32 != 0, got != 0
    clear = ~amb
    excused = amb | (cov32 != cov64)
    both32 = clear & cov64 & cov32
    e32 = float(np.abs(d32.astype(F64) - d64)[both32].max()) if both32.any() else 0.0
    both = clear & cov64 & covg
    eg = float(np.abs(got.astype(F64) - d64)[both].max()) if both.any() else 0.0
    miss = int((clear & (covg != cov64)).sum())
    print(f'{what}: covered {cov64.mean():.3f}, excused {amb.mean():.5f} (with float32 numpy disagreements {excused.mean():.5f}, cap {CAP_PIXELS}), '
          f'coverage mismatches {miss}, depth error {eg:.3e} (float32 numpy {e32:.3e}, bound {4 * e32:.3e})')
    assert excused.mean() <= CAP_PIXELS, excused.mean()
    assert miss == 0, miss
    assert eg <= 4 * e32, (eg, e32)


# ---- 1. raster ---------------------------------------------------------------------------------------------------------------
def run_raster(lib, device, verts, faces, c2w, cam):
    s = SceneDepth(dev(verts, device), dev(faces, device, np.int32), c2w, _lib=lib, **cam)
    assert tuple(s.depth.shape) == (cam['H'], cam['W']) and s.depth.dtype == torch.float32
    return s


def check_raster(lib, device, name, W, H, cull, moved, full=False):
    verts, faces, c2w, cam, d64, amb, d32 = raster_case(name, W, H, cull, moved, full)
    got = run_raster(lib, device, verts, faces, c2w, cam).depth.cpu().numpy()
    compare_depth(got, d64, amb, d32, f'raster {name} {cam["W"]}x{cam["H"]} cull={int(cull)} moved={int(moved)}')
    if name in ('full', 'hd'):
        assert (d64 != 0).all()                              # the big-triangle launch reached every pixel
    return got


def check_raster_independence(lib, device, name, W, H):
    verts, faces, c2w, cam = raster_case(name, W, H, True, False)[:4]
    a = run_raster(lib, device, verts, faces, c2w, cam).depth
    b = run_raster(lib, device, verts, faces, c2w, cam).depth
    perm = np.random.default_rng(3).permutation(len(faces))
    c = run_raster(lib, device, verts, faces[perm], c2w, cam).depth
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert bool((a != 0).any())


# ---- 2. query ----------------------------------------------------------------------------------------------------------------
def scene_mesh(cam, seed):
    """a slab in front of the left part of the image at 1.6-1.9 m plus a few random triangles: about half the pixels stay empty"""
    W, H = cam['W'], cam['H']
    q = np.stack([_backproject(-4.0, 0.1 * H, 1.6, cam), _backproject(0.55 * W, 0.13 * H, 1.9, cam),
                  _backproject(0.52 * W, 0.93 * H, 1.8, cam), _backproject(-5.0, 0.9 * H, 1.7, cam)]).astype(F32)
    slab = (q, face_camera(q, np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
    rv, rf = random_triangles(10, seed, cam, radius_px=6.0, zlo=1.2, zhi=1.5)
    return join(slab, (rv, face_camera(rv, rf)))


def body_sequence(T, F, seed, cam):
    """a 'body' of F triangles at 2-3 m drifting over T frames: verts [T, 3 F, 3], faces [F, 3]"""
    v0, faces = random_triangles(F, seed, cam, radius_px=7.0, zlo=2.0, zhi=3.0)
    rng = np.random.default_rng(seed + 1)
    drift = np.cumsum(rng.standard_normal((T, 1, 3)) * 0.02, 0)
    return (v0[None] + drift).astype(F32), faces


def query_points(verts, faces, P, seed, cam):
    """P points per frame: centroids of body triangles pushed a little (many land on covered pixels), free points over the image,
    and -- from P >= 25 -- the edge cases in fixed slots: outside the image on all four sides, u in (-1, 0), Z = 0, behind the camera"""
    rng = np.random.default_rng(seed)
    T = verts.shape[0]
    pts = np.zeros((T, P, 3), F64)
    for t in range(T):
        f = faces[rng.integers(0, len(faces), P)]
        w = rng.dirichlet(np.ones(3), P)
        pts[t] = (verts[t][f].astype(F64) * w[..., None]).sum(1)
        free = rng.random(P) < 0.3
        z = rng.uniform(1.0, 4.0, P)
        pts[t][free] = _backproject(rng.uniform(0, cam['W'], P), rng.uniform(0, cam['H'], P), z, cam)[free]
    if P >= 25:
        W, H = cam['W'], cam['H']
        special = [_backproject(-7.3, 0.5 * H + 0.37, 2.0, cam), _backproject(W + 3.4, 0.4 * H + 0.41, 2.0, cam), _backproject(0.3 * W + 0.29, -2.6, 2.0, cam),
                   _backproject(0.6 * W + 0.23, H + 1.2, 2.0, cam), _backproject(-0.4, 0.35 * H + 0.31, 2.5, cam), np.array([0.1, 0.2, 0.0]),
                   np.array([0.0, 0.0, 0.0]), np.array([0.2, -0.1, -1.5])]
        pts[:, :len(special)] = np.asarray(special)
    return pts.astype(F32)


@functools.lru_cache(maxsize=None)
def query_scene(W, H):
    cam = camera(W, H)
    verts, faces = scene_mesh(cam, 40 + W)
    d64, amb = restate_raster(verts, faces, None, cam, F64)
    d32, _ = restate_raster(verts, faces, None, cam, F32, want_amb=False)
    return cam, verts, faces, d64, amb, d32


@functools.lru_cache(maxsize=None)
def query_case(T, P, F, W, H):
    """inputs and both restatements, computed once.  With T P of 25 or 67 a single query near an edge is over the 2 % cap, so the
    seed is moved on until the RESTATEMENTS (float64 flags, float32 numpy disagreements -- nothing of the code under test) stay
    inside it; compare_query asserts the cap."""
    cam, _, _, d64, amb, d32 = query_scene(W, H)
    pfx, pfy = proj_of(cam)
    thresh = float(F32(0.1))
    for attempt in range(16):
        verts, faces = body_sequence(T, F, 1000 * T + 10 * P + F + 7919 * attempt, cam)
        pts = query_points(verts, faces, P, 77 + T + P + F + 7919 * attempt, cam)
        r64 = restate_query(verts, faces, pts, cam, False, pfx, pfy, lambda x, y: (d64[y, x], amb[y, x]), thresh, F64)
        r32 = restate_query(verts, faces, pts, cam, False, pfx, pfy, lambda x, y: (d32[y, x], amb[y, x]), thresh, F32)
        if (r64['amb'] | (r32['mask'] != r64['mask'])).mean() <= CAP_QUERIES:
            break
    return verts, faces, pts, pfx, pfy, thresh, r64, r32


def compare_query(got_mask, got_depth, got_pix, r64, r32, what):
    clear = ~r64['amb']
    excused = r64['amb'] | (r32['mask'] != r64['mask'])
    bits = int((clear & (got_mask != r64['mask'])).sum())
    cov = int((clear & ((got_depth != 0) != (r64['depth_body'] != 0))).sum())
    both32 = clear & (r64['depth_body'] != 0) & (r32['depth_body'] != 0)
    e32 = float(np.abs(r32['depth_body'].astype(F64) - r64['depth_body'])[both32].max()) if both32.any() else 0.0
    both = clear & (r64['depth_body'] != 0) & (got_depth != 0)
    eg = float(np.abs(got_depth.astype(F64) - r64['depth_body'])[both].max()) if both.any() else 0.0
    pixbad = int((clear & ((got_pix[..., 0] != r64['x']) | (got_pix[..., 1] != r64['y']))).sum())
    print(f'{what}: occluded {1 - r64["mask"].mean():.3f}, body covers {(r64["depth_body"] != 0).mean():.3f}, in image {r64["inimg"].mean():.3f}, '
          f'excused {r64["amb"].mean():.4f} (with float32 numpy disagreements {excused.mean():.4f}, cap {CAP_QUERIES}), wrong bits {bits}, '
          f'wrong coverage {cov}, wrong pixels {pixbad}, depth error {eg:.3e} (float32 numpy {e32:.3e}, bound {4 * e32:.3e})')
    assert excused.mean() <= CAP_QUERIES, excused.mean()
    assert bits == 0 and cov == 0 and pixbad == 0
    assert eg <= 4 * e32, (eg, e32)
    assert set(np.unique(got_mask)) <= {0.0, 1.0}


def check_query(lib, device, T, P, F, W=64, H=48, chunk=512):
    cam, sv, sf, d64, amb, d32 = query_scene(W, H)
    scene = run_raster(lib, device, sv, sf, None, cam)
    compare_depth(scene.depth.cpu().numpy(), d64, amb, d32, 'query scene')
    verts, faces, pts, pfx, pfy, thresh, r64, r32 = query_case(T, P, F, W, H)
    masker = OcclusionMasker(scene, faces, thresh=thresh, proj_fx=pfx, proj_fy=pfy, cull_backface=False, chunk=chunk)
    mask, depth, pix = masker(dev(verts, device), dev(pts, device), return_depth=True, return_pixels=True)
    assert tuple(mask.shape) == (T, P) and mask.dtype == torch.float32 and tuple(pix.shape) == (T, P, 2)
    compare_query(mask.cpu().numpy(), depth.cpu().numpy(), pix.cpu().numpy(), r64, r32, f'query T={T} P={P} F={F}')
    assert torch.equal(masker(dev(verts, device), dev(pts, device)), mask)                 # without the optional outputs
    if P >= 25:
        m, px = mask.cpu().numpy(), pix.cpu().numpy()
        assert (m[:, [0, 1, 2, 3, 5, 6]] == 1).all()          # outside on the four sides, Z = 0 twice
        assert (px[:, 4, 0] == 0).all() and (px[:, 0, 0] < 0).all() and (px[:, 1, 0] >= W).all() and (px[:, 2, 1] < 0).all() and (px[:, 3, 1] >= H).all()
        assert (px[:, 5] == NOPIX).all() and (px[:, 6] == NOPIX).all()
    if T > 1:                                                 # frames in launches of 2: the same bits
        again = OcclusionMasker(scene, faces, thresh=thresh, proj_fx=pfx, proj_fy=pfy, cull_backface=False, chunk=2)
        assert torch.equal(again(dev(verts, device), dev(pts, device)), mask)
    return r64


def check_query_designed(lib, device, W=64, H=48):
    """hand-placed geometry with known answers: a pair at thresh +- 1e-2, body without scene, scene without body, the image's
    edges, column 0 from u in (-1, 0), Z = 0"""
    cam = camera(W, H)
    P_ = lambda u, v, z: _backproject(u, v, z, cam)
    zs, th = 2.0, float(F32(0.1))
    sq = np.stack([P_(-3.0, 5.0, zs), P_(40.0, 5.0, zs), P_(40.0, 40.0, zs), P_(-3.0, 40.0, zs)]).astype(F32)
    sfaces = face_camera(sq, np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    tri = lambda u, v, z, r=4.0: [P_(u - r, v - r, z), P_(u + r, v - r, z), P_(u, v + r, z)]
    body = np.asarray(tri(15.4, 20.6, zs + th + 1e-2) + tri(30.4, 20.6, zs + th - 1e-2) + tri(52.4, 20.6, 3.0) + tri(0.4, 30.6, 3.0), F64).astype(F32)
    bfaces = face_camera(body, np.arange(12, dtype=np.int32).reshape(4, 3))
    pts = np.asarray([P_(15.4, 20.6, zs + th + 1e-2),       # 0: scene 0.11 m in front of the body          -> occluded
                      P_(30.4, 20.6, zs + th - 1e-2),       # 1: scene 0.09 m in front                       -> visible
                      P_(52.4, 20.6, 3.0),                  # 2: body, no scene (scene pixel 0)              -> visible
                      P_(22.4, 33.6, 3.0),                  # 3: scene, the body does not cover the pixel    -> visible
                      P_(-0.6, 30.6, 3.0),                  # 4: u in (-1, 0): column 0, scene 1 m in front  -> occluded
                      P_(-1.6, 30.6, 3.0), P_(W + 0.4, 20.3, 3.0), P_(20.3, -0.7, 3.0), P_(20.3, H + 0.2, 3.0),      # 5-8: outside
                      [0.1, 0.1, 0.0]], F64).astype(F32)[None]                                                       # 9: Z = 0
    pfx, pfy = cam['fx'], cam['fy']                          # the render's own intrinsics: the points sit where they were placed
    scene = run_raster(lib, device, sq, sfaces, None, cam)
    d64, amb = restate_raster(sq, sfaces, None, cam, F64)
    for cull in (True, False):
        masker = OcclusionMasker(scene, bfaces, thresh=th, proj_fx=pfx, proj_fy=pfy, cull_backface=cull)
        mask, depth, pix = masker(dev(body[None], device), dev(pts, device), return_depth=True, return_pixels=True)
        m, d, px = mask.cpu().numpy()[0], depth.cpu().numpy()[0], pix.cpu().numpy()[0]
        print('designed query: mask', m.tolist(), 'depth', d.tolist(), 'pixels', px.tolist())
        assert m.tolist() == [0, 1, 1, 1, 0, 1, 1, 1, 1, 1]
        assert px[:5].tolist() == [[15, 20], [30, 20], [52, 20], [22, 33], [0, 30]] and px[5, 0] == -1 and px[6, 0] == W and px[7, 1] == 0
        assert px[8, 1] == H and px[9].tolist() == [NOPIX, NOPIX]
        assert abs(d[0] - 2.11) < 1e-5 and abs(d[1] - 2.09) < 1e-5 and abs(d[2] - 3) < 1e-5 and d[3] == 0 and abs(d[4] - 3) < 1e-5 and (d[5:] == 0).all()
        r64 = restate_query(body[None], bfaces, pts, cam, cull, pfx, pfy, lambda x, y: (d64[y, x], amb[y, x]), th, F64)
        assert not r64['amb'].any() and np.array_equal(r64['mask'][0], m)
    # wound the other way the body is culled: no body depth anywhere, everything visible
    masker = OcclusionMasker(scene, bfaces[:, [0, 2, 1]], thresh=th, proj_fx=pfx, proj_fy=pfy, cull_backface=True)
    mask, depth = masker(dev(body[None], device), dev(pts, device), return_depth=True)
    assert bool((mask == 1).all()) and bool((depth == 0).all())


def check_query_equals_raster(lib, device, W=64, H=48, T=3, P=67, F=300):
    """the two halves of the reference's own formulation: the query's body depth IS the body's rendered depth at that pixel"""
    cam, sv, sf = query_scene(W, H)[:3]
    scene = run_raster(lib, device, sv, sf, None, cam)
    verts, faces = body_sequence(T, F, 31, cam)
    pts = query_points(verts, faces, P, 32, cam)
    pfx, pfy = proj_of(cam)
    n = 0
    for cull in (False, True):
        masker = OcclusionMasker(scene, faces, proj_fx=pfx, proj_fy=pfy, cull_backface=cull)
        _, depth, pix = masker(dev(verts, device), dev(pts, device), return_depth=True, return_pixels=True)
        depth, pix = depth.cpu().numpy(), pix.cpu().numpy()
        for t in range(T):
            img = render_depth(dev(verts[t], device), dev(faces, device, np.int32), _lib=lib, **dict(cam, cull_backface=cull)).cpu().numpy()
            x, y = pix[t, :, 0], pix[t, :, 1]
            inimg = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            want = np.where(inimg, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(F32)
            assert np.array_equal(depth[t].view(np.int32), want.view(np.int32))
            n += int((want != 0).sum())
    assert n > 50, n                                           # the comparison saw covered pixels


# ---- 3. full size (GPU) ------------------------------------------------------------------------------------------------------
def room(cam):
    """floor 1 m below the camera (20 x 20 cells) and a box 0.3 m ahead that hides the left part of what stands behind it, outward-facing, in camera coordinates"""
    gx, gz = np.meshgrid(np.linspace(-3, 3, 21), np.linspace(0.5, 8, 21), indexing='ij')
    fv = np.stack([gx, np.full_like(gx, 1.0), gz], -1).reshape(-1, 3)
    idx = np.arange(21 * 21).reshape(21, 21)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    ff = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)])
    n = np.cross(fv[ff[:, 1]] - fv[ff[:, 0]], fv[ff[:, 2]] - fv[ff[:, 0]])
    ff[n[:, 1] > 0] = ff[n[:, 1] > 0][:, [0, 2, 1]]           # normals up (-y)
    lo, hi = np.array([-0.2, -0.1, 0.25]), np.array([-0.03, 0.15, 0.35])
    bv = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    bf = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    n = np.cross(bv[bf[:, 1]] - bv[bf[:, 0]], bv[bf[:, 2]] - bv[bf[:, 0]])
    out = ((bv[bf].mean(1) - (lo + hi) / 2) * n).sum(-1) < 0
    bf[out] = bf[out][:, [0, 2, 1]]
    return join((fv.astype(F32), ff.astype(np.int32)), (bv.astype(F32), bf.astype(np.int32)))


def synthetic_body(lib, device, T, seed=0):
    """T frames of the SMPL-X-shaped synthetic model (V = 10475, F = 20908) 1.3 m in front of the camera, where it fills the image"""
    from lemo_amd import synthetic
    from lemo_amd.body_model import create
    model = synthetic.make_synthetic_smplx(seed=0)
    assert model['f'].shape == (20908, 3)
    # the model's own faces are random index triples: body-sized triangles, thousands of them over every pixel, whose edge lines
    # would put a third of the queries within 1e-3 px of an edge.  Same V and F, triangles of a body mesh's size instead.
    model['f'] = synthetic.local_faces(model['v_template'], 20908)
    bm = create(model, batch_size=T, _lib=lib).to(device)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(device)
    transl = torch.tensor([-0.2, 0.0, 1.3]) + torch.randn(T, 3, generator=g) * torch.tensor([0.1, 0.03, 0.05])
    with torch.no_grad():
        out = bm(global_orient=r(T, 3, k=0.3), body_pose=r(T, 63, k=0.15), transl=transl.to(device), betas=r(T, 10, k=0.5))
    return bm, out


def check_full_size(lib, device, T=4):
    from lemo_amd.assets import load_vertex_ids
    cam = camera(0, 0, True, full=True)
    sv, sf = room(cam)
    c2w = rigid(8)
    world = (sv.astype(F64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)
    xf = np.linalg.inv(c2w)[:3].astype(F32)
    scene = SceneDepth(dev(world, device), dev(sf, device, np.int32), c2w, _lib=lib)          # the module's defaults ARE this camera
    sdepth = scene.depth.cpu().numpy()
    ids = np.asarray(load_vertex_ids()['markers67'], np.int64)
    # 20908 triangles stacked in depth put some 30 bounding boxes over every pixel of the body, and T P is only 100 and 268: the
    # pose seed is moved on until the RESTATEMENTS of both point sets are inside the 2 % cap (nothing of the code under test decides)
    for seed in range(12):
        bm, out = synthetic_body(lib, device, T, seed)
        assert tuple(out.vertices.shape) == (T, 10475, 3) and bm.faces.shape == (20908, 3)
        verts = out.vertices.cpu().numpy()
        sets = []
        for what, points in (('joints', out.joints[:, :25].contiguous()), ('markers', out.vertices[:, torch.from_numpy(ids).to(device)].contiguous())):
            pts = points.cpu().numpy()
            # the scene at the queried pixels and their 3 x 3 neighbourhoods
            _, _, x, y, inimg = project(pts, cam, 1060.53, 1060.53, F64)
            nb = np.array([(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)])
            qx = np.clip(x[inimg][:, None] + nb[:, 0], 0, cam['W'] - 1).ravel()
            qy = np.clip(y[inimg][:, None] + nb[:, 1], 0, cam['H'] - 1).ravel()
            s64, samb = restate_at(world, sf, xf, cam, qx, qy, F64)
            s32, _ = restate_at(world, sf, xf, cam, qx, qy, F32, want_amb=False)
            table = {(int(a), int(b)): (c, d, e) for a, b, c, d, e in zip(qx, qy, s64, samb, s32)}
            at = lambda k, table=table: (lambda px, py: tuple(np.array([table[(int(a), int(b))][i] for a, b in zip(px, py)]) for i in k))
            r64 = restate_query(verts, bm.faces, pts, cam, True, 1060.53, 1060.53, at((0, 1)), 0.1, F64)
            r32 = restate_query(verts, bm.faces, pts, cam, True, 1060.53, 1060.53, at((2, 1)), 0.1, F32)
            sets.append((what, points, (qx, qy, s64, samb, s32), r64, r32))
        if all((r64['amb'] | (r32['mask'] != r64['mask'])).mean() <= CAP_QUERIES for _, _, _, r64, r32 in sets):
            break
    print('full size: pose seed', seed)
    masker = OcclusionMasker(scene, bm.faces)
    for (what, points, (qx, qy, s64, samb, s32), r64, r32), got in zip(sets, (masker.joints(out), masker.markers(out, ids))):
        P = points.shape[1]
        assert tuple(got.shape) == (T, P) and P == (25 if what == 'joints' else 67)
        mask, depth, pix = masker(out.vertices, points, return_depth=True, return_pixels=True)
        assert torch.equal(mask, got)
        compare_depth(sdepth[qy, qx], s64, samb, s32, f'full-size scene around the {what}')
        compare_query(mask.cpu().numpy(), depth.cpu().numpy(), pix.cpu().numpy(), r64, r32, f'full size {what} T={T}')
        assert r64['inimg'].mean() > 0.8 and 0.02 < 1 - r64['mask'].mean() < 0.98      # the box hides a part of the body, not all


# ---- 4. hand-over ------------------------------------------------------------------------------------------------------------
def check_hand_over(lib, device, tmp_path, full, B=100):
    """a [B, 67] mask from masker.markers drives a PROX window in place of the synthetic one, and feeds the trainer's loader"""
    import __graft_entry__ as G
    from lemo_amd.infill_train import load_prox_mask_clips
    prob = G.prox_full_problem('S3', B=B, D=64) if full else G.prox_small_problem(B=B, real_markers=True)
    engine, bm = G.prox_engine_for(dict(prob, infill={}), device, lib=lib)        # only for its body model
    del engine
    p = {k: dev(v, device, F32) for k, v in prob['params'].items()}
    with torch.no_grad():
        out = bm(global_orient=p['global_orient'], body_pose=torch.zeros(B, 63, device=device), transl=p['transl'], betas=p['betas'],
                 left_hand_pose=p['left_hand_pose'], right_hand_pose=p['right_hand_pose'])
    cam = camera(0, 0, True, full=True)
    wall = np.stack([_backproject(-50, -50, 1.5, cam), _backproject(951, -50, 1.5, cam), _backproject(951, 1130, 1.5, cam),
                     _backproject(-50, 1130, 1.5, cam)]).astype(F32)            # hides what projects left of the image's centre
    scene = SceneDepth(dev(wall, device), face_camera(wall, np.array([[0, 1, 2], [0, 2, 3]], np.int32)), _lib=lib)
    mask = OcclusionMasker(scene, bm.faces, cull_backface=False).markers(out, prob['ids']['markers67'])
    rate = float(mask.mean())
    print(f'hand-over: [{B}, 67] mask, visible {rate:.3f}')
    assert tuple(mask.shape) == (B, 67) and mask.device == out.vertices.device and 0.05 < rate < 0.95
    infill = dict(prob['infill'], marker_mask=mask)
    engine, _ = G.prox_engine_for(dict(prob, infill=infill), device, lib=lib)
    assert engine.use_infill and engine._t['mask'].data_ptr() == mask.data_ptr()           # taken as it is, on the device
    engine.step(1, use_graph=False)
    losses = engine.loss_dict()
    print('hand-over: one step on the device-made mask', losses)
    assert all(np.isfinite(float(v)) for v in losses.values())
    os.makedirs(tmp_path / 'masks' / 'seq_a')
    np.save(tmp_path / 'masks' / 'seq_a' / 'mask_markers.npy', mask.cpu().numpy())
    L = B // 4
    clips = load_prox_mask_clips(str(tmp_path / 'masks'), clip_len=L)
    assert clips.shape == (4, L, 201) and set(np.unique(clips)) <= {0.0, 1.0}
    assert np.array_equal(clips[0][:, ::3], mask.cpu().numpy()[:L])


# ---- 5. validation -----------------------------------------------------------------------------------------------------------
def check_validation(lib, device, monkeypatch):
    cam = camera(64, 48)
    sv, sf = scene_mesh(cam, 1)
    scene = run_raster(lib, device, sv, sf, None, cam)
    verts, faces = body_sequence(2, 20, 3, cam)
    pts = query_points(verts, faces, 5, 4, cam)
    V, P, Fd = dev(verts, device), dev(pts, device), dev(faces, device, np.int32)
    launched = []
    for name in ('depth_raster', 'occlusion_query'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    other = torch.device('cpu') if device.type != 'cpu' else None
    bad_raster = [dict(verts=V), dict(verts=V[0].double()), dict(verts=V[0][:, :2]), dict(faces=Fd.long()), dict(faces=Fd[:, :2]),
                  dict(faces=faces.astype(np.float32)), dict(faces=faces + 60), dict(faces=-faces - 1), dict(verts=verts[0]),
                  dict(W=0), dict(H=0), dict(W=40000), dict(fx=0.0), dict(znear=0.0), dict(zfar=0.01), dict(cx=float('nan')),
                  dict(transform=np.eye(3)), dict(transform=np.full((4, 4), np.inf))]
    if other is not None:
        bad_raster += [dict(verts=V[0].to(other)), dict(faces=Fd.to(other))]
    for kw in bad_raster:
        args = dict(dict(verts=V[0], faces=Fd, _lib=lib), **{k: v for k, v in cam.items()})
        args.update(kw)
        with pytest.raises((ValueError, _hip.LemoHipError)):
            render_depth(**args)
    with pytest.raises(ValueError):
        SceneDepth(V[0], Fd, np.eye(3), _lib=lib, **cam)
    for kw in (dict(thresh=float('nan')), dict(proj_fx=0.0), dict(proj_fy=-1.0), dict(chunk=0), dict(chunk=70000)):
        with pytest.raises(ValueError):
            OcclusionMasker(scene, faces, **kw)
    for bad in (faces.astype(np.float64), faces[:, :2], -faces - 1, Fd.long(), 'scene'):
        with pytest.raises((ValueError, _hip.LemoHipError)):
            OcclusionMasker(*((bad, faces) if isinstance(bad, str) else (scene, bad)))
    masker = OcclusionMasker(scene, faces)
    big = torch.zeros(2, 129, 3, device=device)
    bad_query = [(V[0], P), (V, P[0]), (V, P[:1]), (V.double(), P), (V, P.double()), (V[:, :30], P), (V, big), (V, P[:, :0]), (V, P[..., :2]),
                 (verts, P), (V, pts)]
    if other is not None:
        bad_query += [(V.to(other), P), (V, P.to(other))]
    for v, p in bad_query:
        with pytest.raises((ValueError, _hip.LemoHipError)):
            masker(v, p)
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    c = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 1)
    q = lambda cam_=c, T=1, V_=3, F=1, P_=1, ws=1, verts_=1: lib.occlusion_query(verts_, T, V_, 1, F, 1, P_, C.byref(cam_), 60.0, 60.0, 1, 0.1, ws, 1, None, None, None)
    assert q(P_=129) == 10001 and q(P_=0) == 10001 and q(T=0) == 10001 and q(T=65536) == 10001 and q(F=0) == 10001 and q(V_=0) == 10001
    assert q(ws=None) == 10002 and q(verts_=None) == 10002
    assert lib.depth_raster(None, 3, 1, 1, None, C.byref(c), 1, None) == 10002 and lib.depth_raster(1, 3, 1, 1, None, C.byref(c), None, None) == 10002
    assert lib.depth_raster(1, 0, 1, 1, None, C.byref(c), 1, None) == 10001 and lib.depth_raster(1, 3, 1, 1, None, None, 1, None) == 10002
    for k, v, code in (('W', 0, 10001), ('H', 0, 10001), ('W', 40000, 10001), ('znear', 0.0, 10002), ('fx', 0.0, 10002), ('zfar', 0.01, 10002)):
        b = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 1)
        setattr(b, k, v)
        assert q(cam_=b) == code and lib.depth_raster(1, 3, 1, 1, None, C.byref(b), 1, None) == code
