"""The cases of the scene-view tests (lemo_amd.scene_view, csrc/view_kernels.hip), shared by the emulator suite
(tests/test_scene_view_emu.py) and the GPU suite (tests/test_scene_view_gpu.py).  Every figure is printed before it is asserted.

THE YARDSTICK IS NEITHER PYRENDER NOR OPEN3D (neither is installed where this project is built).  It is a numpy restatement of the
five rules lemo_amd/scene_view.py documents, evaluated in float64 and again in float32 operation by operation, on top of the raster
restatement of occlusion_common (_setup with its transform, _hits, _rays, _cross) and the normals, quantisation and face groups of
render_common -- imported, not copied.  The spheres are restated by trying EVERY sphere at EVERY pixel: the kernel's screen bound and
its per-tile lists are no part of the rule.  In the float64 evaluation the transformed vertices the normals are computed from pass
through float32 once (render_common.restate_normals takes float32 vertices); coverage, depth and ids use the float64 transform.

Excused from exact comparison ("ambiguous") is a pixel
  * that render_common excuses within the scene or within the body: within 1e-3 px of an edge of a triangle whose bounding box
    contains it, two hits of one layer within TIE_REL relative Z, float32 and float64 disagreeing on the id or the coverage,
  * within 1e-3 px of the silhouette of a sphere that is drawn (|disc| < 1e-3 |grad disc| per pixel, float64),
  * whose two nearest hits among different layers, or among different spheres, differ by less than TIE_REL relative Z, or
  * on whose owner the float32 and float64 restatements disagree.
Spheres with the same centre and radius bits are ONE surface under two indices (their Z coincides in any arithmetic): the lowest
index must own, exactly, and the "second-nearest sphere" is the nearest of another surface.
AT MOST 2 % OF THE COVERED PIXELS of a case may be excused (CAP_COVERED), asserted on the restatements alone; where a seed lands
over the cap the seed is moved on (nothing of the code under test decides).  Outside the excused pixels owner and coverage are
exact, depth is within 4 x the float32 restatement's own largest error on the case, rgb within 1 level of the float64 restatement.
"""
import functools
import struct

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd.occlusion import render_depth
from lemo_amd.render import BodyRenderer
from lemo_amd.scene_view import SceneView, load_ply, look_at
from occlusion_common import F32, F64, _backproject, _cross, _hits, _rays, _setup, camera, dev, face_camera, join, random_triangles, rigid
from render_common import CAP_COVERED, SHADE, TIE_REL, all_pixels, bumpy_sphere, face_groups, quantise, restate_normals, same_bits

SIZES = ((64, 48), (67, 45))
SIL_PX = 1e-3
YELLOW, STEEL, GREEN, RED = (218, 165, 32), (70, 130, 180), (0, 128, 0), (128, 0, 0)    # vis_opt_amass.py's marker colours


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def xf32(*mats):
    """rule 1: the product of the given [4, 4] (None = identity) in float64, rounded once -> float32 [3, 4], None if all are None"""
    mats = [np.asarray(m, F64) for m in mats if m is not None]
    if not mats:
        return None
    m = mats[0]
    for k in mats[1:]:
        m = m @ k
    return m[:3].astype(F32)


def transform(points, xf, dt):
    """rule 1 in dtype dt: ((m0 x + m1 y) + m2 z) + m3 per row"""
    v = np.asarray(points, F32).astype(dt)
    if xf is None:
        return v
    m = np.asarray(xf, F32).astype(dt)
    with np.errstate(all='ignore'):
        return np.stack([((m[k, 0] * v[..., 0] + m[k, 1] * v[..., 1]) + m[k, 2] * v[..., 2]) + m[k, 3] for k in range(3)], -1)


def layer_pixels(verts, faces, xf, cam, px, py, par, dt, colors=None, lit=True, want_near=True, chunk=4096):
    """a mesh layer (rules 2 and 3) at the pixels (px, py) -> dict(depth (inf = none), id (-1 = none), z2 (nearest hit of another surface),
    rgb uint8 [N, 3], near).  colors None: the body (base colour x shade); else the scene (interpolated vertex colours x shade)."""
    S = _setup(verts, faces, xf, cam, dt)
    f = np.asarray(faces, np.int64)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    N = len(px)
    dx, dy = _rays(px, py, cam, dt)
    flaggable = S['live'] & ~((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
    live = np.nonzero(S['live'])[0]
    near = np.zeros(N, bool)
    P, Fi, Z = [], [], []
    for lo in range(0, len(live), chunk):
        idx = live[lo:lo + chunk]
        b = S['box'][idx]
        k, p = np.nonzero((px >= b[:, 0:1]) & (px <= b[:, 1:2]) & (py >= b[:, 2:3]) & (py <= b[:, 3:4]))
        if not len(k):
            continue
        fi = idx[k]
        z, nr = _hits(S, fi, dx[p][:, None], dy[p][:, None], cam, dt, want_near)
        z = z[:, 0]
        if want_near:
            np.logical_or.at(near, p, nr[:, 0] & flaggable[fi])
        hit = np.isfinite(z) & S['draw'][fi]
        P.append(p[hit]); Fi.append(fi[hit]); Z.append(z[hit])
    P, Fi, Z = (np.concatenate(a) if a else np.zeros(0, t) for a, t in ((P, np.int64), (Fi, np.int64), (Z, dt)))
    order = np.lexsort((Fi, Z, P))                            # per pixel: nearest first, ties to the lowest face index
    P, Fi, Z = P[order], Fi[order], Z[order]
    first = np.nonzero(np.r_[True, P[1:] != P[:-1]])[0] if len(P) else np.zeros(0, np.int64)
    depth, fid, z2 = np.full(N, np.inf, dt), np.full(N, -1, np.int64), np.full(N, np.inf, dt)
    depth[P[first]], fid[P[first]] = Z[first], Fi[first]
    grp = face_groups(faces)
    other = grp[Fi] != grp[fid[P]]
    np.minimum.at(z2, P[other], Z[other])
    cov = np.nonzero(fid >= 0)[0]
    g = fid[cov]
    E = S['E'][g]
    e = [(E[:, i, 0] * dx[cov] + E[:, i, 1] * dy[cov]) + E[:, i, 2] for i in range(3)]
    with np.errstate(all='ignore'):
        s = (e[0] + e[1]) + e[2]
        bw = [e[i] / s for i in range(3)]
        sh = np.ones(len(cov), dt)
        if lit:
            _, unit = restate_normals(transform(verts, xf, dt), faces, dt)
            nv = [unit[f[g, i]] for i in range(3)]
            n = (bw[0][:, None] * nv[0] + bw[1][:, None] * nv[1]) + bw[2][:, None] * nv[2]
            ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            lam = np.where(ln > 0, np.abs(n[:, 2]) / ln, dt(0))
            sh = np.minimum(dt(1), dt(F32(par['ambient'])) + dt(F32(par['diffuse'])) * lam).astype(dt)
        if colors is None:
            col = np.stack([dt(F32(bk)) * sh for bk in par['base_color']], -1)
        else:
            C = (np.asarray(colors, np.uint8).astype(F32) / F32(255)).astype(dt)
            cv = [C[f[g, i]] for i in range(3)]
            col = ((bw[0][:, None] * cv[0] + bw[1][:, None] * cv[1]) + bw[2][:, None] * cv[2]) * sh[:, None]
    rgb = np.zeros((N, 3), np.uint8)
    rgb[cov] = quantise(col.astype(dt))
    return dict(depth=depth, id=fid, z2=z2, rgb=rgb, near=near, grp=grp)


def sphere_groups(centres, radius):
    """[P] -> the lowest index among the spheres with the same centre and radius bits"""
    key = np.concatenate([np.asarray(centres, F32), np.asarray(radius, F32)[:, None]], 1).view(np.uint32)
    low = {}
    return np.array([low.setdefault(tuple(k), i) for i, k in enumerate(key)], np.int64)


def sphere_pixels(centres, radius, colors, xf, cam, px, py, par, dt):
    """rule 4 at the pixels: EVERY sphere at EVERY pixel -> dict(depth (inf = none), s (-1 = none; the lowest index among the nearest),
    z2 (nearest hit of another surface), rgb uint8 [N, 3], near (the silhouette flag))"""
    N = len(px)
    out = dict(depth=np.full(N, np.inf, dt), s=np.full(N, -1, np.int64), z2=np.full(N, np.inf, dt), rgb=np.zeros((N, 3), np.uint8),
               near=np.zeros(N, bool))
    if centres is None:
        return out
    c = transform(centres, xf, dt)                              # [P, 3]
    r = np.asarray(radius, F32).astype(dt)
    znear, zfar = dt(cam['znear']), dt(cam['zfar'])
    with np.errstate(all='ignore'):
        drawn = np.isfinite(c).all(-1) & np.isfinite(r) & (r > 0) & ~(c[:, 2] - r < znear)
    dx, dy = _rays(np.asarray(px, np.int64), np.asarray(py, np.int64), cam, dt)
    d = np.stack([dx, dy, np.ones_like(dx)], -1)[None]           # [1, N, 3]
    cb = c[:, None, :]
    with np.errstate(all='ignore'):
        A = (dx * dx + dy * dy) + dt(1)
        q = _cross(cb, d)                                       # [P, N, 3]
        qq = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        disc = A[None] * (r * r)[:, None] - qq
        Z = (((dx[None] * cb[..., 0] + dy[None] * cb[..., 1]) + cb[..., 2]) - np.sqrt(disc)) / A[None]
        hit = drawn[:, None] & (disc >= 0) & (Z >= znear) & (Z <= zfar)
        # the silhouette: disc = 0; distance in pixels ~ |disc| / |gradient of disc per pixel|
        gx = (dt(2) * dx[None] * (r * r)[:, None] - dt(2) * (q[..., 1] * cb[..., 2] - q[..., 2] * cb[..., 1])) / dt(cam['fx'])
        gy = (dt(2) * dy[None] * (r * r)[:, None] - dt(2) * (q[..., 2] * cb[..., 0] - q[..., 0] * cb[..., 2])) / dt(cam['fy'])
        out['near'] = (drawn[:, None] & ~(np.abs(disc) >= SIL_PX * np.hypot(gx, gy))).any(0)
    Z = np.where(hit, Z, np.inf)
    s = Z.argmin(0)                                             # the first of equal minima: the lowest index
    z = Z[s, np.arange(N)]
    any_hit = np.isfinite(z)
    grp = sphere_groups(centres, radius)
    out['z2'] = np.where(grp[:, None] != grp[s][None, :], Z, np.inf).min(0)
    out['depth'], out['s'] = z, np.where(any_hit, s, -1)
    cs = c[s]                                                   # [N, 3] centre of each pixel's sphere
    with np.errstate(all='ignore'):
        n0, n1, n2 = z * dx - cs[:, 0], z * dy - cs[:, 1], z - cs[:, 2]
        ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        lam = np.where(ln > 0, np.abs(n2) / ln, dt(0))
        sh = np.minimum(dt(1), dt(F32(par['ambient'])) + dt(F32(par['diffuse'])) * lam).astype(dt)
        C = (np.asarray(colors, np.uint8).astype(F32) / F32(255)).astype(dt)[s]
        rgb = quantise((C * sh[:, None]).astype(dt))
    out['rgb'] = np.where(any_hit[:, None], rgb, 0).astype(np.uint8)
    return out


def restate_frame(case, b, px, py, dt):
    """rules 1 - 5 for frame b at the pixels -> dict(owner, depth (0 = none), rgb, amb (what this evaluation alone can flag), name)"""
    cam, par = case['cam'], case['par']
    N = len(px)
    inf = np.full(N, np.inf, dt)
    none = dict(depth=inf, id=np.full(N, -1, np.int64), z2=inf, rgb=np.zeros((N, 3), np.uint8), near=np.zeros(N, bool), grp=np.zeros(1, np.int64))
    want_near = dt is F64
    body = layer_pixels(case['verts'][b], case['faces'], xf32(case['view']), cam, px, py, par, dt, want_near=want_near)
    scene = none
    if case['scene'] is not None:
        sv, sf, sc = case['scene']
        scene = layer_pixels(sv, sf, xf32(case['view'], case['scene_xf']), cam, px, py, par, dt, colors=sc, lit=case['lit'], want_near=want_near)
    sph = sphere_pixels(None, None, None, None, cam, px, py, par, dt)
    if case['spheres'] is not None:
        cols = case['sphere_colors'] if case['sphere_colors'].ndim == 2 else case['sphere_colors'][b]
        sph = sphere_pixels(case['spheres'][b], case['radius'], cols, xf32(case['view']), cam, px, py, par, dt)
    zb, zs, zc = body['depth'], sph['depth'], scene['depth']
    # nearest wins; equal: body, spheres, scene
    is_body = np.isfinite(zb) & (zb <= zs) & (zb <= zc)
    is_sph = ~is_body & np.isfinite(zs) & (zs <= zc)
    is_scene = ~is_body & ~is_sph & np.isfinite(zc)
    owner = np.where(is_body, 1, np.where(is_sph, 2 + sph['s'], np.where(is_scene, 0, -1)))
    depth = np.where(is_body, zb, np.where(is_sph, zs, np.where(is_scene, zc, dt(0)))).astype(dt)
    bg = np.asarray(case['bg'], np.uint8)
    rgb = np.where(is_body[:, None], body['rgb'], np.where(is_sph[:, None], sph['rgb'], np.where(is_scene[:, None], scene['rgb'], bg[None])))
    # the surface that owns the pixel, up to the names of coincident faces
    name = np.where(is_body, body['grp'][np.maximum(body['id'], 0)], np.where(is_scene, scene['grp'][np.maximum(scene['id'], 0)], -1))
    z = np.sort(np.stack([zb, body['z2'], zs, sph['z2'], zc, scene['z2']]), 0)
    with np.errstate(all='ignore'):
        tie = np.isfinite(z[1]) & (z[1] - z[0] < TIE_REL * z[0])
    amb = tie | body['near'] | scene['near'] | sph['near']
    return dict(owner=owner, depth=depth, rgb=rgb.astype(np.uint8), amb=amb, name=name)


def restate_both(case, b, px, py):
    """-> (r64, r32, excused, covered, excused fraction of the covered)"""
    r64, r32 = restate_frame(case, b, px, py, F64), restate_frame(case, b, px, py, F32)
    amb = r64['amb'] | (r32['owner'] != r64['owner']) | (r32['name'] != r64['name'])
    cov = r64['owner'] >= 0
    return r64, r32, amb, cov, float((amb & cov).sum() / max(int(cov.sum()), 1))


# ---- cases -------------------------------------------------------------------------------------------------------------------
def to_world(p_cam, c2w):
    """camera-space points -> world (float64 on the host, rounded once); what the view then undoes"""
    p = np.asarray(p_cam, F64)
    with np.errstate(all='ignore'):
        return (p @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)


def scene_quad(cam):
    """a large tilted quad across the left two thirds of the image that cuts through the body (Z 1.8 .. 2.25 against 2 +- 0.5)"""
    W, H = cam['W'], cam['H']
    q = np.stack([_backproject(-3.0, 0.1 * H, 1.8, cam), _backproject(0.7 * W, 0.05 * H, 2.25, cam),
                  _backproject(0.72 * W, 0.93 * H, 2.2, cam), _backproject(-4.0, 0.9 * H, 1.85, cam)]).astype(F32)
    return q, face_camera(q, np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def special_spheres(cam, B, P, seed):
    """camera-space centres [B, P, 3] and radii [P], at least 4 px each.  The first slots (as many as P allows) hold, in this order:
    0 crossing the body's silhouette, 1 + 2 intersecting each other, 3 half outside the image, 4 a NaN centre, 5 behind the
    camera, 6 c_z - r < znear, 7 r = 0, 8 in front of the quad, 9 behind the quad, 10 + 11 identical, 12 an infinite radius;
    the rest are random.  The frames drift by a few millimetres."""
    rng = np.random.default_rng(seed)
    W, H = cam['W'], cam['H']
    px_r = lambda n_px, z: n_px * z / cam['fx']
    rows = [(_backproject(0.5 * W + 6.3, 0.5 * H - 2.2, 1.62, cam), px_r(5.0, 1.62)),
            (_backproject(0.8 * W + 0.4, 0.25 * H + 0.3, 1.7, cam), px_r(5.5, 1.7)),
            (_backproject(0.8 * W + 4.9, 0.25 * H + 2.1, 1.75, cam), px_r(4.5, 1.75)),
            (_backproject(W - 1.3, 0.7 * H, 2.4, cam), px_r(6.0, 2.4)),
            (np.array([np.nan, 0.1, 2.0]), 0.2),
            (np.array([0.1, -0.1, -1.5]), 0.3),
            (np.array([0.02, 0.01, 0.1]), 0.14),
            (_backproject(0.3 * W, 0.3 * H, 1.5, cam), 0.0),
            (_backproject(0.2 * W + 0.6, 0.5 * H + 0.2, 1.4, cam), px_r(4.2, 1.4)),
            (_backproject(0.35 * W + 0.1, 0.75 * H + 0.4, 2.7, cam), px_r(7.0, 2.7)),
            (_backproject(0.9 * W - 0.2, 0.8 * H + 0.1, 2.1, cam), px_r(4.0, 2.1)),
            (_backproject(0.9 * W - 0.2, 0.8 * H + 0.1, 2.1, cam), px_r(4.0, 2.1)),
            (_backproject(0.1 * W, 0.1 * H, 3.0, cam), np.inf)]
    if P == 1:
        rows = rows[:1]
    elif P < len(rows):
        rows = [rows[i] for i in (0, 1, 2, 3, 4, 10, 11)][:P]
    c = np.stack([r[0] for r in rows])
    rad = np.array([r[1] for r in rows], F64)
    if P > len(rows):                                          # a crowd along the top of the image, behind the others, and one in the open at the end
        n = P - len(rows)
        z = rng.uniform(2.5, 3.5, n)
        u, v = rng.uniform(-3, W + 3, n), rng.uniform(-3, 0.2 * H, n)
        u[-1], v[-1], z[-1] = 0.55 * W + 0.3, 0.9 * H + 0.2, 1.3
        c = np.concatenate([c, _backproject(u, v, z, cam)])
        rad = np.concatenate([rad, z * rng.uniform(4.0, 5.0, n) / cam['fx']])
    drift = np.cumsum(np.random.default_rng(seed + 1).standard_normal((B, 1, 3)) * 0.004, 0)
    return (c[None] + drift), rad.astype(F32)


@functools.lru_cache(maxsize=None)
def view_case(W, H, cull=False, lit=True, colored=True, P=0, moved=True, with_scene=True, B=3, frame_colors=False):
    """inputs (world coordinates, float32) and per-frame restatements over all pixels, computed once and never modified.  The seed is
    moved on until every frame's restatements are inside the 2 % cap."""
    cam = camera(W, H, cull)
    px, py = all_pixels(cam)
    c2w = rigid(5) if moved else None
    sxf = rigid(7) if moved else None                          # the scene's own frame -> world
    put = (lambda p: to_world(p, c2w)) if moved else (lambda p: np.asarray(p, F64).astype(F32))
    for attempt in range(24):
        seed = 900 + 7919 * attempt + W + 3 * P
        rng = np.random.default_rng(seed)
        v0, faces = bumpy_sphere(10, 12, cam, seed)
        drift = np.cumsum(np.random.default_rng(seed + 1).standard_normal((B, 1, 3)) * 0.01, 0)
        drift[0] = 0
        verts = put(v0[None].astype(F64) + drift)
        scene = scene_xf = None
        if with_scene:
            sv, sf = join(random_triangles(300, seed + 2, cam), scene_quad(cam))
            sw = put(sv)
            if moved:                                          # world -> the scene's own frame; scene_transform brings it back
                inv = np.linalg.inv(sxf)
                sw = (sw.astype(F64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
                scene_xf = sxf
            scene = (sw, sf, rng.integers(0, 256, (len(sw), 3), dtype=np.uint8) if colored else None)
        case = dict(cam=cam, par=SHADE, verts=verts, faces=faces, view=np.linalg.inv(c2w) if moved else None, scene=scene, scene_xf=scene_xf,
                    lit=lit, bg=(255, 255, 255), scene_color=(90, 200, 140), spheres=None, radius=None, sphere_colors=None)
        if scene is not None and not colored:
            case['scene'] = (scene[0], scene[1], np.broadcast_to(np.asarray(case['scene_color'], np.uint8), scene[0].shape))
            case['scene_uncolored'] = True
        if P:
            c, rad = special_spheres(cam, B, P, seed + 3)
            case.update(spheres=put(c), radius=rad, sphere_colors=rng.integers(0, 256, (B, P, 3) if frame_colors else (P, 3), dtype=np.uint8))
        frames = [restate_both(case, b, px, py) for b in range(B)]
        if all(fr[4] <= CAP_COVERED for fr in frames):
            break
    print(f'case {W}x{H} cull={int(cull)} lit={int(lit)} colored={int(colored)} P={P} moved={int(moved)}: seed attempt {attempt}, excused of covered '
          f'{[round(fr[4], 4) for fr in frames]}, owners {sorted(set(np.concatenate([fr[0]["owner"] for fr in frames]).tolist()))[:8]} ..')
    case['frames'] = frames
    return case


def make_view(lib, device, case, **kw):
    args = dict(case['cam'], **SHADE)
    args.update(bg_color=case['bg'], scene_lit=case['lit'], view=case['view'], scene_transform=case['scene_xf'], device=device, _lib=lib)
    if case['scene'] is not None:
        args.update(scene_vertices=case['scene'][0], scene_faces=case['scene'][1])
        if case.get('scene_uncolored'):
            args.update(scene_color=case['scene_color'])
        else:
            args.update(scene_colors=case['scene'][2])
    args.update(kw)
    return SceneView(case['faces'], **args)


def run(view, case, device, frames=slice(None)):
    verts = dev(case['verts'][frames], device)
    kw = {}
    if case['spheres'] is not None:
        cols = case['sphere_colors'] if case['sphere_colors'].ndim == 2 else case['sphere_colors'][frames]
        kw = dict(spheres=dev(case['spheres'][frames], device), sphere_radius=dev(case['radius'], device), sphere_colors=dev(cols, device))
    out = view(verts, return_depth=True, return_owner=True, **kw)
    B = verts.shape[0]
    assert out[0].dtype == torch.uint8 and tuple(out[0].shape) == (B, view.H, view.W, 3) and out[0].device == verts.device
    assert out[1].dtype == torch.float32 and out[2].dtype == torch.int32 and all(tuple(t.shape) == (B, view.H, view.W) for t in out[1:])
    return out


def compare(got, frame, what):
    """got = (rgb [N, 3], depth [N], owner [N]) of the code under test at the frame's pixels"""
    rgb, depth, owner = got
    r64, r32, amb, cov, frac = frame
    clear = ~amb
    wrong_cov = int((clear & ((owner >= 0) != cov)).sum())
    wrong_owner = int((clear & (owner != r64['owner'])).sum())
    err = lambda a, m: float(np.abs(a.astype(F64) - r64['depth'])[m].max()) if m.any() else 0.0
    cc = clear & cov
    d32, dg = err(r32['depth'], cc & (r32['owner'] >= 0)), err(depth, cc & (owner >= 0))
    lvl = int(np.abs(rgb[clear].astype(int) - r64['rgb'][clear].astype(int)).max()) if clear.any() else 0
    kinds = {k: int((r64['owner'] == k).sum()) for k in (-1, 0, 1)}
    print(f'{what}: background / scene / body / sphere pixels {kinds[-1]} / {kinds[0]} / {kinds[1]} / {int((r64["owner"] >= 2).sum())}, excused of '
          f'covered {frac:.4f} (cap {CAP_COVERED}), wrong coverage {wrong_cov}, wrong owner {wrong_owner}, depth error {dg:.3e} (float32 numpy '
          f'{d32:.3e}, bound {4 * d32:.3e}), rgb levels from float64 {lvl}')
    assert frac <= CAP_COVERED, frac
    assert wrong_cov == 0 and wrong_owner == 0
    assert dg <= 4 * d32, (dg, d32)
    assert lvl <= 1
    assert ((depth != 0) == (owner >= 0)).all()


def flat(out, b):
    rgb, depth, owner = (t[b].cpu().numpy() for t in out)
    return rgb.reshape(-1, 3), depth.reshape(-1), owner.reshape(-1).astype(np.int64)


# ---- 1. + 2. layers and spheres against the restatement ------------------------------------------------------------------------
def check_layers(lib, device, W, H, cull=False, lit=True, colored=True, P=0, frame_colors=False):
    case = view_case(W, H, cull, lit, colored, P, frame_colors=frame_colors)
    B = case['verts'].shape[0]
    out = run(make_view(lib, device, case, chunk=2), case, device)          # B = 3 with chunk 2: the last chunk holds one frame
    for b in range(B):
        compare(flat(out, b), case['frames'][b], f'view {W}x{H} cull={int(cull)} lit={int(lit)} colored={int(colored)} P={P} frame {b}')
    owners = np.concatenate([fr[0]['owner'] for fr in case['frames']])
    assert (owners == 0).sum() > 50 and (owners == 1).sum() > 50 and (owners == -1).sum() > 50        # the case shows every layer
    return case, out


def check_spheres(lib, device, W, H, P):
    case, out = check_layers(lib, device, W, H, P=P, frame_colors=P == 5)
    owner = out[2].cpu().numpy()
    own64 = np.stack([fr[0]['owner'] for fr in case['frames']]).reshape(owner.shape)
    seen = sorted(set(own64[own64 >= 2].tolist()))
    print(f'spheres P={P}: spheres that own pixels in the restatement {len(seen)} of {P}')
    assert len(seen) >= 1
    if P >= 13:
        # not drawn: NaN centre, behind the camera, c_z - r < znear, r = 0, infinite radius; of two identical ones the first owns
        for s in (4, 5, 6, 7, 11, 12):
            assert not (owner == 2 + s).any() and not (own64 == 2 + s).any(), s
        for s in (0, 1, 2, 3, 8, 10):
            assert (owner == 2 + s).any(), s
        assert max(seen) >= 2 + 128                             # a sphere past the first 128 reaches the image
        quad_front = case['frames'][0][0]['owner'].reshape(H, W)
        assert (quad_front == 2 + 8).sum() > 20
    if P == 5:
        assert not (owner == 2 + 4).any()                       # the NaN centre


# ---- 3. anchors ----------------------------------------------------------------------------------------------------------------
def check_body_only(lib, device, W, H):
    """no scene, no spheres, view None: BodyRenderer(cull_backface=False) over bg_color, image and depth, bit for bit"""
    case = view_case(W, H, P=0, moved=False, with_scene=False)
    cam = dict(case['cam'], cull_backface=False)
    bg = (12, 200, 255)
    view = SceneView(case['faces'], bg_color=bg, device=device, _lib=lib, chunk=2, **dict(cam, **SHADE))
    img, depth, owner = view(dev(case['verts'], device), return_depth=True, return_owner=True)
    B = case['verts'].shape[0]
    back = torch.tensor(bg, dtype=torch.uint8, device=device).expand(B, H, W, 3).contiguous()
    want = BodyRenderer(case['faces'], _lib=lib, **dict(cam, **SHADE))(dev(case['verts'], device), background=back, return_depth=True, return_face_ids=True)
    print(f'body only {W}x{H}: differing rgb bytes {int((img != want[0]).sum())}, differing depth words {int((depth.view(torch.int32) != want[1].view(torch.int32)).sum())}')
    assert torch.equal(img, want[0]) and torch.equal(depth.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(owner, torch.where(want[2] >= 0, 1, -1).to(torch.int32))
    assert bool((owner == 1).any()) and bool((owner == -1).any())


def check_anchors(lib, device, W, H, P=5):
    case = view_case(W, H, P=P, frame_colors=True)
    B = case['verts'].shape[0]
    view = make_view(lib, device, case, chunk=2)
    out = run(view, case, device)
    # the same bits with chunk 1 and 8, in a second run, and for frame 0 alone
    for chunk in (1, 8):
        assert same_bits(run(make_view(lib, device, case, chunk=chunk), case, device), out), chunk
    assert same_bits(run(view, case, device), out)
    assert same_bits(run(view, case, device, slice(0, 1)), [t[:1] for t in out])
    # the depth is the elementwise nearest of render_depth of the transformed scene, of the transformed body and of the kernel's own
    # depth for a spheres-only call (a body of one far-away degenerate triangle: nothing of it is drawn)
    cam = case['cam']
    sv, sf, _ = case['scene']
    near = lambda a, b: torch.where((a != 0) & ((b == 0) | (a < b)), a, b)
    d_scene = render_depth(dev(sv, device), dev(sf, device, np.int32), np.r_[xf32(case['view'], case['scene_xf']), [[0, 0, 0, 1]]], _lib=lib, **cam)
    assert torch.equal((view.scene_key.view(torch.int32) != 0), d_scene != 0)
    none = SceneView(np.array([[0, 0, 0]], np.int32), view=case['view'], device=device, _lib=lib, **dict(cam, **SHADE))
    nobody = torch.full((B, 1, 3), float('nan'), device=device)
    cols = dev(case['sphere_colors'], device)
    d_sph = none(nobody, spheres=dev(case['spheres'], device), sphere_radius=dev(case['radius'], device), sphere_colors=cols, return_depth=True)[1]
    wrong = 0
    for b in range(B):
        d_body = render_depth(dev(case['verts'][b], device), dev(case['faces'], device, np.int32), np.r_[xf32(case['view']), [[0, 0, 0, 1]]], _lib=lib, **cam)
        want = near(near(d_body, d_sph[b]), d_scene)
        wrong += int((want.view(torch.int32) != out[1][b].view(torch.int32)).sum())
    print(f'anchors {W}x{H}: depth words that are not the nearest of the three layers {wrong}')
    assert wrong == 0
    # owner 0 pixels carry the static layer's rgb
    m = out[2] == 0
    assert bool(m.any()) and torch.equal(out[0][m], view.scene_rgb[None].expand(B, H, W, 3)[m])
    assert bool((out[0][out[2] == -1] == 255).all())
    return case, out


def check_permutations(lib, device, W, H, P=130):
    case, out = view_case(W, H, P=P), None
    out = run(make_view(lib, device, case), case, device)
    B = case['verts'].shape[0]
    clear = np.stack([~fr[2] for fr in case['frames']]).reshape(B, H, W)
    # the scene's faces in another order: nothing changes outside the pixels the restatement marks as ties
    sv, sf, sc = case['scene']
    perm = np.random.default_rng(3).permutation(len(sf))
    outp = run(make_view(lib, device, case, scene_faces=sf[perm]), case, device)
    assert torch.equal(out[1].view(torch.int32), outp[1].view(torch.int32)) and torch.equal(out[2], outp[2])
    diff = (out[0] != outp[0]).any(-1).cpu().numpy()
    print(f'permuted scene faces {W}x{H}: rgb differs at {int(diff.sum())} pixels, outside the excused ones at {int((diff & clear).sum())}')
    assert not (diff & clear).any()
    # the spheres in another order: only the owner numbers change
    sp = np.random.default_rng(4).permutation(P)
    moved = dict(case, spheres=case['spheres'][:, sp], radius=case['radius'][sp], sphere_colors=case['sphere_colors'][sp])
    outs = run(make_view(lib, device, case), moved, device)
    o, os_ = out[2].cpu().numpy(), outs[2].cpu().numpy()
    grp = sphere_groups(case['spheres'][0], case['radius'])      # identical spheres: one surface, the lowest index of the ORDER owns
    back = np.where(os_ >= 2, 2 + grp[sp[np.maximum(os_ - 2, 0)]], os_)
    same_rgb = (out[0] == outs[0]).all(-1).cpu().numpy()
    twins = np.isin(o, 2 + np.nonzero(np.bincount(grp, minlength=P) > 1)[0])          # their colours differ with the index that owns
    print(f'permuted spheres {W}x{H}: owner differs at {int((back != np.where(o >= 2, 2 + grp[np.maximum(o - 2, 0)], o)).sum())} pixels, rgb at '
          f'{int((~same_rgb & ~twins).sum())}')
    assert torch.equal(out[1].view(torch.int32), outs[1].view(torch.int32))
    assert (back == np.where(o >= 2, 2 + grp[np.maximum(o - 2, 0)], o)).all() and same_rgb[~twins].all()


# ---- 4. view -------------------------------------------------------------------------------------------------------------------
def check_look_at():
    rng = np.random.default_rng(0)
    for _ in range(6):
        eye, target, up = rng.standard_normal(3), rng.standard_normal(3) * 2, rng.standard_normal(3)
        m = look_at(eye, target, up)
        R = m[:3, :3]
        fwd = R @ (target - eye)
        print(f'look_at: det {np.linalg.det(R):.12f}, |R R^T - 1| {np.abs(R @ R.T - np.eye(3)).max():.2e}, forward {fwd / np.linalg.norm(fwd)}, up -> y {(R @ up)[1]:.3f}')
        assert m.shape == (4, 4) and m.dtype == np.float64 and np.array_equal(m[3], [0, 0, 0, 1])
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        assert np.abs(fwd / np.linalg.norm(fwd) - [0, 0, 1]).max() < 1e-12 and (R @ up)[1] < 0 and abs((R @ up)[0]) < 1e-12 * max(1, np.linalg.norm(up))
        assert np.abs(m @ np.r_[eye, 1] - [0, 0, 0, 1]).max() < 1e-12
    assert np.allclose(look_at([0, 0, 0], [0, 0, 5], [0, -1, 0]), np.eye(4))
    for bad in (([0, 0, 0], [0, 0, 0], [0, -1, 0]), ([0, 0, 0], [0, 0, 1], [0, 0, 2]), ([0, 0, np.nan], [0, 0, 1], [0, 1, 0]), ([0, 0], [0, 0, 1], [0, 1, 0])):
        with pytest.raises(ValueError):
            look_at(*bad)


def check_set_view(lib, device, W, H):
    case = view_case(W, H, P=5, frame_colors=True)
    c2w = np.linalg.inv(case['view'])
    eye = c2w[:3, 3] + c2w[:3, :3] @ [0.25, -0.2, -0.3]          # a little beside, above and behind the case's camera
    other = look_at(eye, c2w[:3, 3] + c2w[:3, :3] @ [0.0, 0.0, 2.0], -c2w[:3, 1])
    view = make_view(lib, device, case)
    first = run(view, case, device)
    view.set_view(other)
    moved = run(view, case, device)
    fresh = run(make_view(lib, device, case, view=other), case, device)
    print(f'set_view {W}x{H}: pixels whose owner changed with the viewpoint {int((first[2] != moved[2]).sum())}, covered in the new view {int((moved[2] >= 0).sum())}')
    assert same_bits(moved, fresh) and torch.equal(view.scene_rgb, make_view(lib, device, case, view=other).scene_rgb)
    assert bool((first[2] != moved[2]).any()) and all(bool((moved[2] == k).any()) for k in (-1, 0, 1))
    view.set_view(case['view'])
    assert same_bits(run(view, case, device), first)
    # view . scene_transform: the same bits as a scene that was brought into the world in float64 on the host, with the product
    # of the two handed over as the view and no scene_transform (the composition happens once, in float64, either way)
    sv, sf, sc = case['scene']
    both = case['view'] @ case['scene_xf']
    a = make_view(lib, device, case)
    b = make_view(lib, device, case, view=None, scene_transform=both)
    assert torch.equal(a.scene_key, b.scene_key) and torch.equal(a.scene_rgb, b.scene_rgb)
    # and pre-transforming the scene's vertices on the host in float64 gives the restatement's scene up to the rounding of the vertices
    pre = (sv.astype(F64) @ both[:3, :3].T + both[:3, 3]).astype(F32)
    c = make_view(lib, device, case, scene_vertices=pre, view=None, scene_transform=None)
    cam = case['cam']
    px, py = all_pixels(cam)
    clear = ~np.any([fr[2] for fr in case['frames']], 0).reshape(H, W)
    cov_a, cov_c = (a.scene_key != 0).cpu().numpy(), (c.scene_key != 0).cpu().numpy()
    lvl = np.abs(a.scene_rgb.cpu().numpy().astype(int) - c.scene_rgb.cpu().numpy().astype(int)).max(-1)
    print(f'pre-transformed scene {W}x{H}: coverage differs at {int((cov_a != cov_c).sum())} pixels, outside the excused ones at '
          f'{int(((cov_a != cov_c) & clear).sum())}; rgb levels apart there {int(lvl[clear & cov_a & cov_c].max())}')
    assert not ((cov_a != cov_c) & clear).any() and lvl[clear & cov_a & cov_c].max() <= 1


# ---- 5. load_ply ---------------------------------------------------------------------------------------------------------------
def write_ply(path, verts, faces, colors=None, binary=False, extra=False, count_type='uchar', index_type='int', endian='little', index_name='vertex_indices'):
    head = ['ply', f'format {"binary_" + endian + "_endian" if binary else "ascii"} 1.0', 'comment written by the scene-view tests',
            f'element vertex {len(verts)}', 'property float x', 'property float y']
    if extra:
        head.append('property float quality')                   # between y and z: skipped by its declared size
    head.append('property float z')
    if colors is not None:
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    head += [f'element face {len(faces)}', f'property list {count_type} {index_type} {index_name}', 'end_header']
    data = ('\n'.join(head) + '\n').encode()
    e = '<' if endian == 'little' else '>'
    ct, it = {'uchar': 'B', 'int': 'i'}[count_type], {'int': 'i', 'uint': 'I', 'short': 'h'}[index_type]
    for i, v in enumerate(verts):
        vals = [v[0], v[1]] + ([0.25 * i] if extra else []) + [v[2]]
        if binary:
            data += struct.pack(e + 'f' * len(vals), *vals) + (bytes(colors[i].tolist()) if colors is not None else b'')
        else:
            data += (' '.join(repr(float(x)) for x in vals) + ('' if colors is None else ' ' + ' '.join(str(int(c)) for c in colors[i])) + '\n').encode()
    for f in faces:
        if binary:
            data += struct.pack(e + ct, len(f)) + struct.pack(e + it * len(f), *[int(i) for i in f])
        else:
            data += (' '.join(str(int(i)) for i in [len(f), *f]) + '\n').encode()
    with open(path, 'wb') as fh:
        fh.write(data)


def check_load_ply(tmp_path):
    rng = np.random.default_rng(2)
    verts = rng.standard_normal((7, 3)).astype(F32)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    colors = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    n = 0
    for binary in (False, True):
        for col in (None, colors):
            for extra in (False, True):
                for count_type, index_type, name in (('uchar', 'int', 'vertex_indices'), ('int', 'uint', 'vertex_index'), ('uchar', 'short', 'vertex_indices')):
                    p = tmp_path / f'm{n}.ply'
                    n += 1
                    write_ply(p, verts, faces, col, binary, extra, count_type, index_type, index_name=name)
                    v, f, c = load_ply(str(p))
                    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(v, verts) and np.array_equal(f, faces), p
                    assert (c is None) if col is None else (c.dtype == np.uint8 and np.array_equal(c, colors)), p
    print(f'load_ply: {n} files read back exactly')
    bad = tmp_path / 'bad.ply'
    quad = [[0, 1, 2, 3]]
    for kw in (dict(faces=quad), dict(faces=quad, binary=True), dict(faces=faces, binary=True, endian='big'), dict(faces=faces + 7)):
        write_ply(bad, verts, kw.pop('faces'), **kw)
        with pytest.raises(ValueError):
            load_ply(str(bad))
    head = 'ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n'
    for text in (head, head.replace('element vertex 1', 'element face 0\nproperty list uchar int vertex_indices\nelement vertex 1').replace('property float z\n', ''),
                 'not a ply file\n', head.replace('end_header\n', 'element face 1\nproperty list uchar int vertex_indices\nend_header\n')):
        bad.write_bytes(text.encode())
        with pytest.raises(ValueError):
            load_ply(str(bad))


# ---- 6. validation -------------------------------------------------------------------------------------------------------------
def check_validation(lib, device, monkeypatch):
    cam = camera(64, 48)
    v0, faces = random_triangles(20, 3, cam)
    sv, sf = scene_quad(cam)
    sc = np.zeros((4, 3), np.uint8)
    verts = np.stack([v0, v0])
    V = dev(verts, device)
    sph = torch.zeros(2, 5, 3, device=device)
    cols = torch.zeros(5, 3, dtype=torch.uint8, device=device)
    launched = []
    for name in ('vertex_normals', 'render_ids', 'view_transform', 'view_scene_resolve', 'view_compose'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    mk = lambda **kw: SceneView(faces, **dict(dict(cam, **SHADE), device=device, _lib=lib, **kw))
    shear = np.eye(4); shear[0, 1] = 0.3
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    nan = np.eye(4); nan[1, 3] = np.nan
    proj = np.eye(4); proj[3, 2] = 0.1
    for kw in (dict(chunk=0), dict(chunk=70000), dict(fx=0.0), dict(znear=0.0), dict(W=0), dict(H=40000), dict(ambient=1.5), dict(diffuse=float('nan')),
               dict(base_color=(1.0, 1.0)), dict(bg_color=(256, 0, 0)), dict(bg_color=(1, 2)), dict(bg_color=(0.5, 0, 0)),
               dict(scene_faces=sf), dict(scene_colors=sc), dict(scene_vertices=sv), dict(scene_vertices=sv, scene_faces=sf + 2),
               dict(scene_vertices=sv, scene_faces=sf.astype(np.float32)), dict(scene_vertices=sv[:, :2], scene_faces=sf),
               dict(scene_vertices=sv, scene_faces=sf, scene_colors=sc[:3]), dict(scene_vertices=sv, scene_faces=sf, scene_colors=sc.astype(np.float32)),
               dict(scene_vertices=sv, scene_faces=sf, scene_color=(300, 0, 0)), dict(scene_vertices=torch.from_numpy(sv).double(), scene_faces=sf),
               dict(view=shear), dict(view=mirror), dict(view=nan), dict(view=proj), dict(view=np.eye(3)), dict(view=2 * np.eye(4)),
               dict(scene_transform=nan), dict(scene_transform=np.eye(3)), dict(scene_transform=proj)):
        with pytest.raises((ValueError, _hip.LemoHipError)):
            mk(**kw)
    view = mk(scene_vertices=sv, scene_faces=sf, scene_colors=sc)
    assert launched == ['vertex_normals', 'render_ids', 'view_scene_resolve']
    launched.clear()
    for bad in (shear, nan, np.eye(3)):
        with pytest.raises(ValueError):
            view.set_view(bad)
    other = torch.device('cpu') if device.type != 'cpu' else None
    good = dict(vertices=V, spheres=sph, sphere_colors=cols)
    bad_calls = [dict(vertices=V[0]), dict(vertices=V.double()), dict(vertices=V[..., :2]), dict(vertices=verts), dict(vertices=V[:, :30]),
                 dict(spheres=sph[:1]), dict(spheres=sph.double()), dict(spheres=sph[0]), dict(spheres=sph[..., :2]), dict(spheres=sph[:, :0]),
                 dict(spheres=sph.cpu().numpy()), dict(spheres=torch.zeros(2, 257, 3, device=device), sphere_colors=torch.zeros(257, 3, dtype=torch.uint8, device=device)),
                 dict(sphere_radius=torch.zeros(4, device=device)), dict(sphere_radius=torch.zeros(5, 1, device=device)), dict(sphere_radius=torch.zeros(5, dtype=torch.float64, device=device)),
                 dict(sphere_radius=np.zeros(6, np.float32)), dict(sphere_colors=None), dict(sphere_colors=cols[:4]), dict(sphere_colors=cols.float()),
                 dict(sphere_colors=torch.zeros(3, 5, 3, dtype=torch.uint8, device=device)), dict(sphere_colors=torch.zeros(5, 4, dtype=torch.uint8, device=device))]
    if other is not None:
        bad_calls += [dict(vertices=V.to(other)), dict(spheres=sph.to(other))]
    for kw in bad_calls:
        with pytest.raises((ValueError, _hip.LemoHipError)):
            view(**dict(good, **kw))
    assert launched == []
    view.set_view(look_at([0, 0, -0.5], [0, 0, 2], [0, -1, 0]))
    view(**good, sphere_radius=[0.1, 0.2, 0.1, 0.2, 0.3])                # and a good call reaches every entry point
    assert launched == ['view_transform', 'vertex_normals', 'render_ids', 'view_scene_resolve', 'view_transform', 'vertex_normals', 'render_ids',
                        'view_compose']
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    import ctypes as C
    SHAPE, ARG = 10001, 10002
    c = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 0)
    sh = _hip.RenderShade((C.c_float * 3)(1.0, 1.0, 0.9), 0.3, 0.7)
    ident = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    inf = (C.c_float * 12)(1, 0, 0, float('inf'), 0, 1, 0, 0, 0, 0, 1, 0)
    assert lib.view_transform(None, 3, ident, 1, None) == ARG and lib.view_transform(1, 3, None, 1, None) == ARG and lib.view_transform(1, 3, ident, None, None) == ARG
    assert lib.view_transform(1, 3, inf, 1, None) == ARG and lib.view_transform(1, 0, ident, 1, None) == SHAPE and lib.view_transform(1, 2 ** 31, ident, 1, None) == SHAPE
    res = lambda verts_=1, nrm=1, V_=3, F=1, cam_=c, ids=1, col=1, amb_=0.3, lit=1, rgb=1: lib.view_scene_resolve(
        verts_, nrm, V_, 1, F, C.byref(cam_) if cam_ else None, ids, col, amb_, 0.7, lit, rgb, None)
    assert res(verts_=None) == ARG and res(nrm=None) == ARG and res(ids=None) == ARG and res(col=None) == ARG and res(rgb=None) == ARG and res(cam_=None) == ARG
    assert res(amb_=1.5) == ARG and res(amb_=float('nan')) == ARG and res(V_=0) == SHAPE and res(F=0) == SHAPE
    cmp_ = lambda verts_=1, nrm=1, B=1, V_=3, F=1, cam_=c, keys=1, ids=1, sh_=sh, sk=None, sr=None, sph_=None, P=0, rad=None, col=None, view_=None, bg=0xFFFFFF, rgb=1: \
        lib.view_compose(verts_, nrm, B, V_, 1, F, C.byref(cam_) if cam_ else None, keys, ids, C.byref(sh_) if sh_ else None, sk, sr, sph_, P, rad, col, 1,
                         view_, bg, rgb, None, None, None)
    assert cmp_(verts_=None) == ARG and cmp_(nrm=None) == ARG and cmp_(keys=None) == ARG and cmp_(ids=None) == ARG and cmp_(sh_=None) == ARG and cmp_(rgb=None) == ARG
    assert cmp_(cam_=None) == ARG and cmp_(bg=0x1000000) == ARG and cmp_(sk=1) == ARG and cmp_(sr=1) == ARG and cmp_(view_=inf) == ARG
    assert cmp_(P=1) == ARG and cmp_(P=1, sph_=1, rad=1) == ARG and cmp_(P=257, sph_=1, rad=1, col=1) == SHAPE and cmp_(P=-1) == SHAPE
    assert cmp_(B=0) == SHAPE and cmp_(B=65536) == SHAPE and cmp_(V_=0) == SHAPE and cmp_(F=0) == SHAPE
    assert cmp_(sh_=_hip.RenderShade((C.c_float * 3)(1.0, 2.0, 0.9), 0.3, 0.7)) == ARG
    for k, v, code in (('W', 0, SHAPE), ('H', 40000, SHAPE), ('znear', 0.0, ARG), ('fx', 0.0, ARG)):
        b = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 0)
        setattr(b, k, v)
        assert cmp_(cam_=b) == code and res(cam_=b) == code


# ---- 7. full size (GPU) ----------------------------------------------------------------------------------------------------------
def big_room(cam, cells=100):
    """a floor of cells x cells quads (2 cells^2 triangles) 1 m below the camera, in camera coordinates, coloured like a checker board"""
    gx, gz = np.meshgrid(np.linspace(-3, 3, cells + 1), np.linspace(0.6, 7, cells + 1), indexing='ij')
    fv = np.stack([gx, 1.0 + 0.02 * np.sin(3 * gx) * np.cos(2 * gz), gz], -1).reshape(-1, 3)
    idx = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    ff = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int32)
    ii, jj = np.divmod(np.arange(len(fv)), cells + 1)
    col = np.stack([60 + 150 * ((ii // 4 + jj // 4) % 2), 90 + (ii * 3) % 120, 200 - (jj * 2) % 150], -1).astype(np.uint8)
    return fv.astype(F32), ff, col


def check_full_size(lib, device, T=2, n_cov=2048, n_unc=512):
    from lemo_amd.assets import load_vertex_ids
    from occlusion_common import synthetic_body
    cam = camera(0, 0, False, full=True)
    W, H = cam['W'], cam['H']
    c2w, sxf = rigid(5), rigid(7)
    ids81 = np.asarray(load_vertex_ids()['markers81'], np.int64)
    assert len(ids81) == 81
    sv, sf, sc = big_room(cam)
    assert len(sf) == 20000
    inv = np.linalg.inv(sxf)
    sw = (to_world(sv, c2w).astype(F64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    rng = np.random.default_rng(11)
    for seed in range(12):
        bm, out = synthetic_body(lib, device, T, seed)
        vc = out.vertices.cpu().numpy()
        faces = np.asarray(bm.faces, np.int32)
        assert vc.shape == (T, 10475, 3) and faces.shape == (20908, 3)
        front = vc[..., 2].min() - 0.05 * (1 + np.arange(81) % 4)
        case = dict(cam=cam, par=SHADE, verts=to_world(vc, c2w), faces=faces, view=np.linalg.inv(c2w), scene=(sw, sf, sc), scene_xf=sxf, lit=True,
                    bg=(255, 255, 255), spheres=to_world(np.concatenate([vc[:, ids81, :2], np.broadcast_to(front[None, :, None], (T, 81, 1))], -1), c2w), radius=np.full(81, 0.02, F32),
                    sphere_colors=np.where((np.arange(81) % 2 == 0)[:, None], YELLOW, STEEL).astype(np.uint8))
        # (the synthetic model's marker vertices lie inside its 2 m deep vertex cloud: the spheres keep their x and y and float in
        # four layers in front of the cloud, where they can be seen)
        # the body fills the image at 1.3 m; pull the camera back so that the floor and the background show
        back = np.eye(4); back[2, 3] = 1.4
        case['view'] = back @ case['view']
        pix, frames = [], []
        for t in range(T):
            x, y = rng.integers(0, W, 6 * n_cov // T), rng.integers(0, H, 6 * n_cov // T)
            cov = restate_frame(case, t, x, y, F64)['owner'] >= 0
            keep = np.r_[np.nonzero(cov)[0][:n_cov // T], np.nonzero(~cov)[0][:n_unc // T]]
            pix.append((x[keep], y[keep]))
            frames.append(restate_both(case, t, *pix[t]))
        cov = sum(int(fr[3].sum()) for fr in frames)
        exc = sum(int((fr[2] & fr[3]).sum()) for fr in frames)
        print(f'full size: pose seed {seed}: sampled covered {cov}, excused of covered {exc / max(cov, 1):.4f}')
        if cov == n_cov and exc <= CAP_COVERED * cov:
            break
    assert cov == n_cov and sum(len(p[0]) for p in pix) - cov == n_unc and exc <= CAP_COVERED * cov
    args = dict(scene_vertices=sw, scene_faces=sf, scene_colors=sc, scene_transform=sxf, view=case['view'], cull_backface=False, device=device, _lib=lib)
    view = SceneView(bm.faces, **args)                         # the module's defaults ARE this camera
    kw = dict(spheres=dev(case['spheres'], device), sphere_radius=0.02, sphere_colors=dev(case['sphere_colors'], device), return_depth=True, return_owner=True)
    got = view(dev(case['verts'], device), **kw)
    assert tuple(got[0].shape) == (T, H, W, 3)
    for t in range(T):
        x, y = pix[t]
        g = tuple(a[t].cpu().numpy()[y, x] for a in got)
        compare((g[0], g[1], g[2].astype(np.int64)), frames[t][:4] + (0.0,), f'full size frame {t}')
        own = frames[t][0]['owner']
        assert (own == 0).sum() > 100 and (own == 1).sum() > 100 and (own >= 2).sum() > 3 and (own == -1).sum() > 100
    again = SceneView(bm.faces, chunk=1, **args)(dev(case['verts'], device), **kw)
    assert same_bits(again, got)                                # chunk independence on the whole image


# ---- 8. hand-over --------------------------------------------------------------------------------------------------------------
def check_hand_over(lib, device, B=14, n=None):
    """a PROX window's engine -> write_back -> body_model -> SceneView images with the markers as spheres, nothing through the host"""
    import __graft_entry__ as G
    prob = G.prox_small_problem(B=B, real_markers=True)
    engine, bm = G.prox_engine_for(dict(prob, infill={}), device, lib=lib)
    engine.step(1, use_graph=False)
    engine.write_back(bm)
    p = {k: dev(v, device, F32) for k, v in prob['params'].items()}
    with torch.no_grad():
        out = bm(body_pose=torch.zeros(B, 63, device=device), betas=p['betas'])
    assert torch.equal(bm.transl.detach(), engine.P['transl'])
    n = B if n is None else n                                   # frames of the window that are rendered
    verts = out.vertices[:n].contiguous()
    markers = verts[:, torch.from_numpy(np.asarray(prob['ids']['markers67'], np.int64)).to(device)].contiguous()
    assert isinstance(verts, torch.Tensor) and verts.device.type == device.type and markers.device == verts.device and verts.dtype == torch.float32
    cam = camera(0, 0, False, full=True)
    wall = np.stack([_backproject(-50, -50, 4.0, cam), _backproject(951, -50, 4.0, cam), _backproject(951, 1130, 4.0, cam), _backproject(-50, 1130, 4.0, cam)]).astype(F32)
    view = SceneView(bm.faces, scene_vertices=wall, scene_faces=np.array([[0, 1, 2], [0, 2, 3]], np.int32), scene_color=(120, 130, 140), device=device, _lib=lib)
    cols = torch.tensor([YELLOW if i % 2 else STEEL for i in range(67)], dtype=torch.uint8, device=device)
    img, owner = view(verts, spheres=markers, sphere_radius=0.02, sphere_colors=cols, return_owner=True)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (n, 1080, 1920, 3) and img.device == verts.device
    share = {k: float((owner == k).float().mean()) for k in (-1, 0, 1)}
    spheres = float((owner >= 2).float().mean())
    print(f'hand-over: [{n}, 1080, 1920, 3] image, background {share[-1]:.3f}, wall {share[0]:.3f}, body {share[1]:.3f}, spheres {spheres:.4f}')
    assert share[-1] > 0.2 and share[0] > 0.2 and 0.005 < share[1] < 0.6 and spheres > 1e-4
    assert bool((img[owner == -1] == 255).all())
