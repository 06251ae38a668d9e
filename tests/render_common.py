"""The cases of the body-overlay tests (lemo_amd.render, csrc/render_kernels.hip), shared by the emulator suite
(tests/test_render_emu.py) and the GPU suite (tests/test_render_gpu.py).  Every figure is printed before it is asserted.

THE YARDSTICK IS NOT PYRENDER (see tests/occlusion_common.py: it is not installed where this project is built).  It is a numpy
restatement of the five rules lemo_amd/render.py documents, evaluated in float64 and again in float32, on top of the raster
restatement of occlusion_common (_setup, _hits, _rays are imported, not copied).  Face ids come from tracking the nearest and the
second-nearest hit of every pixel (ties to the lowest face index).

Excused from exact comparison ("ambiguous") is a pixel
  * within 1e-3 px of an edge of a triangle whose bounding box contains it (occlusion_common's `near` flag; a face that names one
    vertex twice is left out of the flag: its normal is computed as exactly 0 in any arithmetic, so it can never be hit),
  * whose two nearest hits differ by less than 1e-5 Z (the float32 restatement's own depth error on these cases is <= 5e-7
    relative, so this is 20 x that), or
  * on whose id or coverage the float32 and float64 restatements disagree.
Faces that name the same three vertices (in any order) are ONE surface under two names: the "second-nearest hit" is the nearest hit
of another vertex set, and a face id is compared through `face_groups` (the lowest index of its vertex set).  The small cases have no
such faces, so for them this is the rule above word for word.  The full-size body has: `synthetic.local_faces` joins every vertex
to its nearest neighbours, mutual neighbours give the same triangle twice, 2195 of its 20908 faces share their vertex set with
another, and their two hits coincide exactly.  Counted as two hits they alone excuse 3.8 % .. 5.9 % of the covered pixels at every
pose seed tried (0 .. 11; the figure is printed) -- over the cap whatever the code under test does.  Counted as one surface those
pixels are not excused at all: coverage, depth, shade and rgb are compared there like anywhere else, the id up to the name.
AT MOST 2 % OF THE COVERED PIXELS of a case may be excused, asserted on the restatements alone; where a seed lands over the cap the
seed is moved on until the restatements are inside it (nothing of the code under test decides).  Outside the excused pixels coverage
and face id are exact, depth is within 4 x the float32 restatement's own largest error (occlusion_common's house rule), shade within
4 x the float32 restatement's largest shade error on the same case, the uint8 image equals the quantisation of the kernel's own
returned shade exactly and is within 1 level of the float64 restatement.  Normals: the error of the unnormalised sum is within 4 x
the float32 restatement's, over the vertices whose float64 |n| is above 1e-6 of the largest.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd.occlusion import render_depth
from lemo_amd.render import BodyRenderer, face_adjacency, vertex_normals
from occlusion_common import (F32, F64, _backproject, _cross, _hits, _rays, _setup, camera, dev, fullscreen_pair, join, near_crossers,
                              random_triangles, synthetic_body)

TIE_REL = 1e-5
CAP_COVERED = 0.02
SHADE = dict(base_color=(1.0, 1.0, 0.9), ambient=0.3, diffuse=0.7)
SIZES = ((64, 48), (67, 45))
SOUPS = ('F1', 'F65', 'F300', 'full', 'near')
SPHERES = ((10, 12, 64, 48), (16, 24, 64, 48), (24, 32, 67, 45))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def restate_normals(verts, faces, dt):
    """rule 1 -> (sums [V, 3], unit [V, 3]) in dtype dt, every addition in the documented order"""
    v = np.asarray(verts, F32).astype(dt)
    V = len(v)
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < V)).all(1)
    fc = np.where(ok[:, None], f, 0)
    p0, p1, p2 = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    c = _cross(p1 - p0, p2 - p0)
    pairs = np.unique(np.stack([f[ok].reshape(-1), np.repeat(np.nonzero(ok)[0], 3)], -1), axis=0)      # sorted by (vertex, face), each once
    sums = np.zeros((V, 3), dt)
    np.add.at(sums, pairs[:, 0], c[pairs[:, 1]])             # unbuffered: in the order of the pairs
    nn = (sums[:, 0] * sums[:, 0] + sums[:, 1] * sums[:, 1]) + sums[:, 2] * sums[:, 2]
    with np.errstate(all='ignore'):
        unit = np.where((nn > 0)[:, None], sums / np.sqrt(nn)[:, None], dt(0))
    return sums, unit.astype(dt)


def quantise(c):
    """rule 4: (int)(255 c + 0.5) clamped to 0 .. 255, a NaN gives 0; in the dtype of c"""
    dt = c.dtype.type
    with np.errstate(all='ignore'):
        q = np.trunc(dt(255) * c + dt(0.5))
    return np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.uint8)


def face_groups(faces):
    """[F] -> the lowest index among the faces that name the same three vertices"""
    key = np.sort(np.asarray(faces, np.int64), 1)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    low = np.full(inv.max() + 1, len(key), np.int64)
    np.minimum.at(low, inv, np.arange(len(key)))
    return low[inv]


def restate_pixels(verts, faces, cam, px, py, par, dt, want_near=True, chunk=4096):
    """rules 2 - 4 at the pixels (px, py) of one frame -> dict(depth (0 = none), id (-1 = none), z2 (second-nearest depth, inf without),
    z2_any (the same counting every face, coincident ones too), shade, rgb uint8 [N, 3] of the covered pixels (0 elsewhere), near).  Only (face, pixel) pairs whose pixel lies in the face's
    bounding box are evaluated, as the kernels do."""
    S = _setup(verts, faces, None, cam, dt)
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
    depth, fid, z2 = np.zeros(N, dt), np.full(N, -1, np.int64), np.full(N, np.inf, dt)
    depth[P[first]], fid[P[first]] = Z[first], Fi[first]
    second = first + 1
    second = second[(second < len(P))]
    second = second[P[second] == P[second - 1]]
    z2_any = z2.copy()
    z2_any[P[second]] = Z[second]
    grp = face_groups(faces)
    other = grp[Fi] != grp[fid[P]]                            # hits of another surface than the pixel's winner
    np.minimum.at(z2, P[other], Z[other])
    # rule 3 for the covered pixels
    cov = np.nonzero(fid >= 0)[0]
    g = fid[cov]
    E = S['E'][g]
    e = [(E[:, i, 0] * dx[cov] + E[:, i, 1] * dy[cov]) + E[:, i, 2] for i in range(3)]
    _, unit = restate_normals(verts, faces, dt)
    with np.errstate(all='ignore'):
        s = (e[0] + e[1]) + e[2]
        bw = [e[i] / s for i in range(3)]
        nv = [unit[f[g, i]] for i in range(3)]
        n = (bw[0][:, None] * nv[0] + bw[1][:, None] * nv[1]) + bw[2][:, None] * nv[2]
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        lam = np.where(ln > 0, np.abs(n[:, 2]) / ln, dt(0))
    amb_, dif_ = dt(F32(par['ambient'])), dt(F32(par['diffuse']))
    sh = np.minimum(dt(1), amb_ + dif_ * lam).astype(dt)
    shade = np.zeros(N, dt)
    shade[cov] = sh
    rgb = np.zeros((N, 3), np.uint8)
    rgb[cov] = quantise(np.stack([dt(F32(bk)) * sh for bk in par['base_color']], -1).astype(dt))
    return dict(depth=depth, id=fid, z2=z2, z2_any=z2_any, shade=shade, rgb=rgb, near=near, grp=grp)


def restate_pair(verts, faces, cam, px, py, par=SHADE):
    """both evaluations and the excused pixels -> (r64, r32, amb, covered, excused fraction of the covered)"""
    r64 = restate_pixels(verts, faces, cam, px, py, par, F64)
    r32 = restate_pixels(verts, faces, cam, px, py, par, F32, want_near=False)
    cov = r64['id'] >= 0
    tie = cov & (r64['z2'] - r64['depth'] < TIE_REL * r64['depth'])
    name = lambda r: np.where(r['id'] >= 0, r64['grp'][np.maximum(r['id'], 0)], -1)
    amb = r64['near'] | tie | (name(r32) != name(r64))
    frac = float((amb & cov).sum() / max(int(cov.sum()), 1))
    return r64, r32, amb, cov, frac


def restate_points(points, radius, W, H):
    """rule 5 -> bool [B, H, W]"""
    out = np.zeros((len(points), H, W), bool)
    for b, pts in enumerate(np.asarray(points, F32)):
        for u, v in pts:
            if not (np.isfinite(u) and np.isfinite(v)):
                continue
            x, y = int(np.trunc(u)), int(np.trunc(v))
            for j in range(-radius, radius + 1):
                for i in range(-radius, radius + 1):
                    if i * i + j * j <= radius * radius and 0 <= x + i < W and 0 <= y + j < H:
                        out[b, y + j, x + i] = True
    return out


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def bumpy_sphere(rings, segs, cam, seed, radius=0.5, z=2.0):
    """closed latitude / longitude sphere with shared vertices and outward winding, its radius jittered by 5 %, centred half a pixel
    off the image centre at Z = z; plus one isolated vertex (the last) and one zero-area face (the last, a vertex named twice)"""
    rng = np.random.default_rng(seed)
    centre = _backproject(cam['W'] / 2 + 0.5, cam['H'] / 2 + 0.5, z, cam)
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segs) / segs
    d = [np.array([0.0, -1.0, 0.0])] + [np.array([np.sin(t) * np.cos(p), -np.cos(t), np.sin(t) * np.sin(p)]) for t in th for p in ph] + [np.array([0.0, 1.0, 0.0])]
    d = np.asarray(d)
    v = centre + d * (radius * (1 + 0.05 * rng.uniform(-1, 1, len(d))))[:, None]
    ring = lambda r, s: 1 + r * segs + s % segs
    south = len(d) - 1
    f = []
    for s in range(segs):
        f.append([0, ring(0, s), ring(0, s + 1)])
        f.append([south, ring(rings - 2, s + 1), ring(rings - 2, s)])
        for r in range(rings - 2):
            f.append([ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)])
            f.append([ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)])
    f = np.asarray(f, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    inward = (n * (v[f].mean(1) - centre)).sum(-1) < 0
    f[inward] = f[inward][:, [0, 2, 1]]
    assert len(v) == (rings - 1) * segs + 2 and len(f) == 2 * segs * (rings - 1)
    v = np.concatenate([v, centre[None] + [[0.3, 0.2, -0.1]]])                  # isolated
    f = np.concatenate([f, [[5, 7, 7]]])                                        # zero area
    return v.astype(F32), f.astype(np.int32)


def make_mesh(name, cam, seed):
    if name.startswith('F'):
        return random_triangles(int(name[1:]), seed, cam)
    if name == 'full':
        return join(fullscreen_pair(cam), random_triangles(20, seed, cam, zlo=1.5, zhi=3.5))
    if name == 'near':
        return join(near_crossers(cam), random_triangles(12, seed, cam))
    rings, segs = (int(s) for s in name[1:].split('x'))      # 'S24x32'
    return bumpy_sphere(rings, segs, cam, seed)


def all_pixels(cam):
    y, x = np.mgrid[0:cam['H'], 0:cam['W']]
    return x.ravel(), y.ravel()


@functools.lru_cache(maxsize=None)
def render_case(name, W, H, cull, B=3):
    """(verts [B, V, 3], faces, cam, per-frame restatements), computed once and never modified.  The frames are one mesh drifting by a
    few centimetres.  The seed is moved on until every frame's restatements are inside the 2 % cap."""
    cam = camera(W, H, cull)
    px, py = all_pixels(cam)
    for attempt in range(24):
        seed = 500 + 7919 * attempt + W + len(name)
        v0, faces = make_mesh(name, cam, seed)
        drift = np.cumsum(np.random.default_rng(seed + 1).standard_normal((B, 1, 3)) * 0.01, 0)
        drift[0] = 0
        verts = (v0[None] + drift).astype(F32)
        frames = [restate_pair(verts[b], faces, cam, px, py) for b in range(B)]
        if all(fr[4] <= CAP_COVERED for fr in frames):
            break
    print(f'case {name} {W}x{H} cull={int(cull)}: seed attempt {attempt}, excused of covered {[round(fr[4], 4) for fr in frames]}')
    return verts, faces, cam, frames


def renderer(lib, faces, cam, **kw):
    return BodyRenderer(faces, _lib=lib, **dict(cam, **dict(SHADE, **kw)))


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def compare_frame(got, frame, what, base=SHADE['base_color']):
    """got = (rgb [N, 3], depth [N], ids [N], shade [N]) of the code under test at the frame's pixels"""
    rgb, depth, ids, shade = got
    r64, r32, amb, cov, frac = frame
    clear = ~amb
    cc = clear & cov
    wrong_cov = int((clear & ((ids >= 0) != cov)).sum())
    grp = r64['grp']
    wrong_id = int((cc & (ids >= 0) & (grp[np.maximum(ids, 0)] != grp[np.maximum(r64['id'], 0)])).sum())
    err = lambda a, b, m: float(np.abs(a.astype(F64) - b)[m].max()) if m.any() else 0.0
    both = cc & (r32['id'] >= 0)
    d32, dg = err(r32['depth'], r64['depth'], both), err(depth, r64['depth'], cc & (ids >= 0))
    s32, sg = err(r32['shade'], r64['shade'], both), err(shade, r64['shade'], cc & (ids >= 0))
    own = quantise(np.stack([F32(bk) * shade.astype(F32) for bk in base], -1).astype(F32))
    covg = ids >= 0
    own_bad = int((rgb[covg] != own[covg]).any(-1).sum())
    lvl = int(np.abs(rgb[cc].astype(int) - r64['rgb'][cc].astype(int)).max()) if cc.any() else 0
    print(f'{what}: covered {cov.mean():.3f}, excused of covered {frac:.4f} (cap {CAP_COVERED}), wrong coverage {wrong_cov}, wrong ids {wrong_id}, '
          f'depth error {dg:.3e} (float32 numpy {d32:.3e}, bound {4 * d32:.3e}), shade error {sg:.3e} (float32 numpy {s32:.3e}, bound '
          f'{4 * s32:.3e}), rgb != quantised own shade at {own_bad}, rgb levels from float64 {lvl}')
    assert frac <= CAP_COVERED, frac
    assert wrong_cov == 0 and wrong_id == 0
    assert dg <= 4 * d32, (dg, d32)
    assert sg <= 4 * s32, (sg, s32)
    assert own_bad == 0 and lvl <= 1
    assert (depth[~covg] == 0).all() and (shade[~covg] == 0).all() and ((depth != 0) == covg).all()


def run(r, verts, device, **kw):
    out = r(dev(verts, device), return_depth=True, return_face_ids=True, return_shade=True, **kw)
    B = verts.shape[0]
    assert out[0].dtype == torch.uint8 and tuple(out[0].shape) == (B, r.H, r.W, 3)
    assert out[1].dtype == torch.float32 and out[2].dtype == torch.int32 and out[3].dtype == torch.float32
    assert all(tuple(t.shape) == (B, r.H, r.W) for t in out[1:])
    return out


def flat(out, b):
    rgb, depth, ids, shade = (t[b].cpu().numpy() for t in out)
    return rgb.reshape(-1, 3), depth.reshape(-1), ids.reshape(-1).astype(np.int64), shade.reshape(-1)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else x.view(torch.int32), y.view(torch.uint8) if y.dtype == torch.uint8 else y.view(torch.int32))
               for x, y in zip(a, b))


# ---- 1. images against the restatement, chunks, runs, anchors -----------------------------------------------------------------
def check_render(lib, device, name, W, H, cull):
    verts, faces, cam, frames = render_case(name, W, H, cull)
    B = verts.shape[0]
    r = renderer(lib, faces, cam, chunk=8)
    out = run(r, verts, device)
    for b in range(B):
        compare_frame(flat(out, b), frames[b], f'render {name} {W}x{H} cull={int(cull)} frame {b}')
    if name == 'full':
        assert bool((out[2] >= 0).all())                      # the big-box launches reached every pixel
    # the same bits with 2 frames per set of launches, in a second run, and for frame 0 alone (B = 1)
    assert same_bits(run(renderer(lib, faces, cam, chunk=2), verts, device), out)
    assert same_bits(run(r, verts, device), out)
    one = run(r, verts[:1], device)
    assert same_bits(one, [t[:1] for t in out])
    # anchors: the depth IS render_depth's, and a pixel's id face rendered alone gives the same depth bits there
    fd = dev(faces, device, np.int32)
    ids0 = out[2][0].cpu().numpy()
    for b in range(B):
        want = render_depth(dev(verts[b], device), fd, _lib=lib, **cam)
        assert torch.equal(out[1][b].view(torch.int32), want.view(torch.int32))
    ys, xs = np.nonzero(ids0 >= 0)
    pick = np.random.default_rng(1).choice(len(ys), min(6, len(ys)), replace=False) if len(ys) else []
    for k in pick:
        alone = render_depth(dev(verts[0], device), dev(faces[ids0[ys[k], xs[k]]][None], device, np.int32), _lib=lib, **cam)
        assert alone[ys[k], xs[k]].view(torch.int32) == out[1][0, ys[k], xs[k]].view(torch.int32)
    return out


def check_permuted_faces(lib, device, name, W, H):
    """faces in another order: depth identical in bits; on the non-excused pixels the same face wins and -- for the triangle soups,
    whose vertices each belong to one face, so that no sum changes its order -- rgb is identical"""
    verts, faces, cam, frames = render_case(name, W, H, True)
    out = run(renderer(lib, faces, cam), verts, device)
    perm = np.random.default_rng(3).permutation(len(faces))
    outp = run(renderer(lib, faces[perm], cam), verts, device)
    assert torch.equal(out[1].view(torch.int32), outp[1].view(torch.int32))
    n = 0
    for b in range(verts.shape[0]):
        clear = ~frames[b][2]
        a, p = flat(out, b), flat(outp, b)
        covered = a[2] >= 0
        assert ((p[2] >= 0) == covered).all()
        m = clear & covered
        assert (perm[p[2][m]] == a[2][m]).all()
        if not name.startswith('S'):
            assert (a[0][clear] == p[0][clear]).all()
        else:
            assert np.abs(a[0][clear].astype(int) - p[0][clear].astype(int)).max() <= 1
        n += int(m.sum())
    assert n > 20, n


# ---- 2. normals ----------------------------------------------------------------------------------------------------------------
def check_normals(lib, device, rings, segs, W, H):
    verts, faces, cam, _ = render_case(f'S{rings}x{segs}', W, H, True)
    V = verts.shape[1]
    start, face = face_adjacency(faces, V)
    valence = np.diff(start)
    print(f'normals S{rings}x{segs}: V {V}, F {len(faces)}, valence {valence.min()} .. {valence.max()}')
    assert valence.max() == segs and valence[V - 1] == 0 and 12 <= valence.max() <= 32
    unit, sums = vertex_normals(dev(verts, device), faces, return_sums=True, _lib=lib)
    assert tuple(unit.shape) == tuple(verts.shape) and unit.dtype == torch.float32
    again = vertex_normals(dev(verts, device), dev(faces, device, np.int32), _lib=lib)
    assert torch.equal(unit.view(torch.int32), again.view(torch.int32))
    one = vertex_normals(dev(verts[1:2], device), faces, _lib=lib)
    assert torch.equal(unit[1:2].view(torch.int32), one.view(torch.int32))
    unit, sums = unit.cpu().numpy(), sums.cpu().numpy()
    for b in range(verts.shape[0]):
        s64, u64 = restate_normals(verts[b], faces, F64)
        s32, u32 = restate_normals(verts[b], faces, F32)
        big = np.linalg.norm(s64, axis=1) > 1e-6 * np.linalg.norm(s64, axis=1).max()
        e32 = float(np.abs(s32.astype(F64) - s64)[big].max())
        eg = float(np.abs(sums[b].astype(F64) - s64)[big].max())
        eu = float(np.abs(unit[b].astype(F64) - u64)[big].max())
        print(f'  frame {b}: sum error {eg:.3e} (float32 numpy {e32:.3e}, bound {4 * e32:.3e}), unit error {eu:.3e}, |unit| - 1 '
              f'{np.abs(np.linalg.norm(unit[b][big].astype(F64), axis=1) - 1).max():.3e}')
        assert eg <= 4 * e32, (eg, e32)
        assert eu <= 1e-5                                      # unit normals of well-conditioned sums: a few float32 roundings
        assert (unit[b][V - 1] == 0).all() and (sums[b][V - 1] == 0).all()          # the isolated vertex: exactly 0
        # the zero-area face (the last one) contributes 0: without it the sums are the same bits
        s_without = vertex_normals(dev(verts[b:b + 1], device), faces[:-1], return_sums=True, _lib=lib)[1].cpu().numpy()[0]
        assert np.array_equal(s_without.view(np.int32), sums[b].view(np.int32))
    assert big.sum() == V - 1


# ---- 3. background -------------------------------------------------------------------------------------------------------------
def check_background(lib, device, W, H):
    verts, faces, cam, frames = render_case('F65', W, H, True)
    B = verts.shape[0]
    rng = np.random.default_rng(5)
    r = renderer(lib, faces, cam, chunk=2)
    plain = run(r, verts, device)
    covered = (plain[2] >= 0).cpu().numpy()
    assert covered.any() and not covered.all()
    assert bool((plain[0].cpu().numpy()[~covered] == 0).all())                   # no background: black
    shared = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    per = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    fl = rng.uniform(-0.1, 1.1, (B, H, W, 3)).astype(F32)                      # also beyond [0, 1]: clamped
    fl[0, 0, 0] = [np.nan, 0.0, 1.0]
    for what, bg, want in (('shared uint8', shared, np.broadcast_to(shared, per.shape)), ('uint8', per, per), ('float32', fl, quantise(fl)),
                           ('shared float32', fl[1], np.broadcast_to(quantise(fl[1]), per.shape))):
        out = run(r, verts, device, background=dev(bg, device))
        img = out[0].cpu().numpy()
        bad_bg = int((img[~covered] != want[~covered]).any(-1).sum())
        bad_body = int((img[covered] != plain[0].cpu().numpy()[covered]).any(-1).sum())
        print(f'background {what} {W}x{H}: uncovered pixels that are not the background {bad_bg}, covered pixels that changed {bad_body}')
        assert bad_bg == 0 and bad_body == 0
        assert same_bits(out[1:], plain[1:])


# ---- 4. points -----------------------------------------------------------------------------------------------------------------
def check_points(lib, device, W, H, radius):
    verts, faces, cam, frames = render_case('F65', W, H, True)
    B = verts.shape[0]
    r = renderer(lib, faces, cam, chunk=2)
    bg = dev(np.random.default_rng(6).integers(0, 200, (H, W, 3), dtype=np.uint8), device)
    plain = r(dev(verts, device), background=bg)
    ids = r(dev(verts, device), return_face_ids=True)[1].cpu().numpy()
    pts = np.zeros((B, 14, 2), F32)
    for b in range(B):
        cy, cx = np.argwhere(ids[b] >= 0)[len(np.argwhere(ids[b] >= 0)) // 2]
        uy, ux = np.argwhere(ids[b] < 0)[len(np.argwhere(ids[b] < 0)) // 3]
        pts[b] = [[cx + 0.4, cy + 0.6], [ux + 0.7, uy + 0.2],                               # on a covered and on an uncovered pixel
                  [0.3, H / 2], [W - 0.2, H / 3], [W / 3, 0.9], [W / 2, H - 0.1],          # the four borders, inside
                  [-0.5, H / 4], [-1.5, H / 5], [W + 0.5, H / 2], [W / 4, -1.2], [W / 5, H + 0.3],      # u in (-1, 0) is column 0; outside
                  [np.nan, 5.0], [7.0, np.inf], [-np.inf, np.nan]]
    color = (250, 3, 77)
    got = r(dev(verts, device), background=bg, points=dev(pts, device), point_radius=radius, point_color=color)
    want = restate_points(pts, radius, W, H)
    img, base = got.cpu().numpy(), plain.cpu().numpy()
    changed = (img != base).any(-1)
    is_col = (img == np.asarray(color, np.uint8)).all(-1)
    print(f'points r={radius} {W}x{H}: pixels in the restated set {int(want.sum())}, of them not in colour {int((want & ~is_col).sum())}, '
          f'changed outside the set {int((changed & ~want).sum())}')
    assert want.sum() >= B * 6 and (is_col[want]).all() and not (changed & ~want).any()
    assert (img[~want] == base[~want]).all()
    for b in range(B):                                          # u in (-1, 0) lands in column 0, (-2, -1) only with a radius
        assert want[b, int(H / 4), 0] and (radius > 0) == bool(want[b, int(H / 5), 0])


# ---- 5. validation -------------------------------------------------------------------------------------------------------------
def check_validation(lib, device, monkeypatch):
    cam = camera(64, 48)
    v0, faces = random_triangles(20, 3, cam)
    verts = np.stack([v0, v0])
    V, Fd = dev(verts, device), dev(faces, device, np.int32)
    bg = torch.zeros(2, 48, 64, 3, dtype=torch.uint8, device=device)
    pts = torch.zeros(2, 5, 2, device=device)
    launched = []
    for name in ('vertex_normals', 'render_ids', 'render_resolve', 'render_points'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    other = torch.device('cpu') if device.type != 'cpu' else None
    for kw in (dict(chunk=0), dict(chunk=70000), dict(fx=0.0), dict(fy=float('nan')), dict(cx=float('inf')), dict(znear=0.0), dict(zfar=0.01),
               dict(W=0), dict(H=40000), dict(ambient=-0.1), dict(ambient=1.5), dict(diffuse=float('nan')), dict(diffuse=2.0),
               dict(base_color=(1.0, 1.0, 1.2)), dict(base_color=(1.0, 1.0)), dict(base_color=(-0.1, 0.5, 0.5))):
        with pytest.raises(ValueError):
            renderer(lib, faces, cam, **kw)
    for bad in (faces.astype(np.float32), faces[:, :2], -faces - 1, Fd.long(), faces[:0]):
        with pytest.raises(ValueError):
            renderer(lib, bad, cam)
    r = renderer(lib, faces, cam)
    bad_calls = [dict(vertices=V[0]), dict(vertices=V.double()), dict(vertices=V[..., :2]), dict(vertices=verts), dict(vertices=V[:, :30]),
                 dict(background=bg[:1]), dict(background=bg.float().double()), dict(background=bg[..., :2]), dict(background=bg[:, :40]),
                 dict(background=bg.to(torch.int32)), dict(background=np.zeros((48, 64, 3), np.uint8)),
                 dict(points=pts[:1]), dict(points=pts.double()), dict(points=pts[0]), dict(points=torch.zeros(2, 5, 3, device=device)),
                 dict(points=pts[:, :0]), dict(points=pts.cpu().numpy()),
                 dict(points=pts, point_radius=-1), dict(points=pts, point_radius=17), dict(points=pts, point_radius=1.5),
                 dict(points=pts, point_color=(256, 0, 0)), dict(points=pts, point_color=(1, 2))]
    if other is not None:
        bad_calls += [dict(vertices=V.to(other)), dict(background=bg.to(other)), dict(points=pts.to(other))]
    for kw in bad_calls:
        with pytest.raises((ValueError, _hip.LemoHipError)):
            r(**dict(dict(vertices=V), **kw))
    for v, f in ((V[0], faces), (V.double(), faces), (V, faces + 60), (V, faces.astype(np.float64)), (verts, faces), (V, Fd.long())):
        with pytest.raises((ValueError, _hip.LemoHipError)):
            vertex_normals(v, f, _lib=lib)
    assert launched == []
    r(V, background=bg, points=pts)                                  # and a good call reaches every entry point
    assert launched == ['vertex_normals', 'render_ids', 'render_resolve', 'render_points']
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    SHAPE, ARG = 10001, 10002
    c = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 1)
    sh = _hip.RenderShade((C.c_float * 3)(1.0, 1.0, 0.9), 0.3, 0.7)
    nrm = lambda verts_=1, B=1, V_=3, F=1, start=1, face=1, nnz=3, out=1, sums=None: lib.vertex_normals(verts_, B, V_, 1, F, start, face, nnz, out, sums, None)
    assert nrm(verts_=None) == ARG and nrm(start=None) == ARG and nrm(face=None) == ARG and nrm(out=None) == ARG
    assert nrm(B=0) == SHAPE and nrm(B=65536) == SHAPE and nrm(V_=0) == SHAPE and nrm(F=0) == SHAPE and nrm(nnz=-1) == SHAPE
    idp = lambda cam_=c, verts_=1, B=1, V_=3, F=1, keys=1, ids=1: lib.render_ids(verts_, B, V_, 1, F, C.byref(cam_) if cam_ else None, keys, ids, None, None)
    assert idp(verts_=None) == ARG and idp(keys=None) == ARG and idp(ids=None) == ARG and idp(cam_=None) == ARG
    assert idp(B=0) == SHAPE and idp(B=65536) == SHAPE and idp(V_=0) == SHAPE and idp(F=0) == SHAPE
    res = lambda cam_=c, sh_=sh, verts_=1, nrm_=1, B=1, ids=1, bg_=None, kind=0, rgb=1: lib.render_resolve(
        verts_, nrm_, B, 3, 1, 1, C.byref(cam_), ids, C.byref(sh_) if sh_ else None, bg_, kind, 0, rgb, None, None, None)
    assert res(verts_=None) == ARG and res(nrm_=None) == ARG and res(ids=None) == ARG and res(rgb=None) == ARG and res(sh_=None) == ARG
    assert res(kind=1) == ARG and res(kind=3, bg_=1) == ARG and res(B=0) == SHAPE
    for field, value in (('ambient', 1.5), ('diffuse', -0.5), ('ambient', float('nan'))):
        bad = _hip.RenderShade((C.c_float * 3)(1.0, 1.0, 0.9), 0.3, 0.7)
        setattr(bad, field, value)
        assert res(sh_=bad) == ARG
    assert res(sh_=_hip.RenderShade((C.c_float * 3)(1.0, 2.0, 0.9), 0.3, 0.7)) == ARG
    for k, v, code in (('W', 0, SHAPE), ('H', 40000, SHAPE), ('znear', 0.0, ARG), ('fx', 0.0, ARG)):
        b = _hip.OcclCam(60.0, 60.0, 32.0, 24.0, 0.05, 100.0, 64, 48, 1)
        setattr(b, k, v)
        assert idp(cam_=b) == code and res(cam_=b) == code
    pnt = lambda pts_=1, B=1, P=1, rad=2, W=64, H=48, col=0xFF0000, rgb=1: lib.render_points(pts_, B, P, rad, W, H, col, rgb, None)
    assert pnt(pts_=None) == ARG and pnt(rgb=None) == ARG and pnt(col=0x1000000) == ARG
    assert pnt(B=0) == SHAPE and pnt(P=0) == SHAPE and pnt(rad=-1) == SHAPE and pnt(rad=17) == SHAPE and pnt(W=0) == SHAPE and pnt(H=40000) == SHAPE


# ---- 6. full size and hand-over (GPU) --------------------------------------------------------------------------------------------
def check_full_size(lib, device, T=4, n_cov=2048, n_unc=512):
    cam = camera(0, 0, True, full=True)
    W, H = cam['W'], cam['H']
    rng = np.random.default_rng(11)
    for seed in range(12):
        bm, out = synthetic_body(lib, device, T, seed)
        verts, faces = out.vertices.cpu().numpy(), np.asarray(bm.faces, np.int32)
        assert verts.shape == (T, 10475, 3) and faces.shape == (20908, 3)
        frames, pix, cand = [], [], []
        for t in range(T):
            # random candidates: the float64 restatement says which are covered
            x, y = rng.integers(0, W, 8 * n_cov // T), rng.integers(0, H, 8 * n_cov // T)
            cand.append((x, y, restate_pixels(verts[t], faces, cam, x, y, SHADE, F64, want_near=False)['id'] >= 0))
        need = n_unc                                          # the body leaves few pixels free in some frames: the others make up for it
        for t in np.argsort([int((~c).sum()) for _, _, c in cand]):
            x, y, c = cand[t]
            take = min(int((~c).sum()), -(-need // (T - len(pix))))
            need -= take
            keep = np.r_[np.nonzero(c)[0][:n_cov // T], np.nonzero(~c)[0][:take]]
            pix.append((t, x[keep], y[keep]))
        pix = [(x, y) for _, x, y in sorted(pix, key=lambda p: p[0])]
        frames = [restate_pair(verts[t], faces, cam, *pix[t]) for t in range(T)]
        cov = sum(int(fr[3].sum()) for fr in frames)
        exc = sum(int((fr[2] & fr[3]).sum()) for fr in frames)
        twice = sum(int((fr[3] & (fr[2] | (fr[0]['z2_any'] - fr[0]['depth'] < TIE_REL * fr[0]['depth']))).sum()) for fr in frames)
        print(f'full size: pose seed {seed}: excused of covered {exc / cov:.4f}; with coincident faces counted as two hits {twice / cov:.4f}')
        if exc <= CAP_COVERED * cov:
            break
    print(f'full size: pose seed {seed}, sampled covered {cov}, uncovered {sum(len(p[0]) for p in pix) - cov}, excused of covered {exc / cov:.4f}')
    assert cov == n_cov and sum(len(p[0]) for p in pix) - cov == n_unc and exc <= CAP_COVERED * cov
    bg = dev(np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8), device)
    r = BodyRenderer(bm.faces, _lib=lib)                      # the module's defaults ARE this camera
    got = r(out.vertices, background=bg, return_depth=True, return_face_ids=True, return_shade=True)
    assert tuple(got[0].shape) == (T, H, W, 3)
    fd = dev(faces, device, np.int32)
    for t in range(T):
        x, y = pix[t]
        g = tuple(a[t].cpu().numpy()[y, x] for a in got)
        fr = frames[t]
        fr = fr[:4] + (0.0,)                                  # the cap was asserted over all sampled pixels above
        compare_frame((g[0], g[1], g[2].astype(np.int64), g[3]), fr, f'full size frame {t}')
        unc = g[2] < 0
        assert (g[0][unc] == bg.cpu().numpy()[y[unc], x[unc]]).all()
        want = render_depth(out.vertices[t].contiguous(), fd, _lib=lib)
        assert torch.equal(got[1][t].view(torch.int32), want.view(torch.int32))


def check_hand_over(lib, device, B=14, n=None):
    """vertices and joints of the project's body model for a PROX window -> one call with the frames and the projected joints"""
    import __graft_entry__ as G
    from lemo_amd.occlusion import PROX_RENDER
    prob = G.prox_small_problem(B=B, real_markers=True)
    engine, bm = G.prox_engine_for(dict(prob, infill={}), device, lib=lib)        # only for its body model
    del engine
    p = {k: dev(v, device, F32) for k, v in prob['params'].items()}
    with torch.no_grad():
        out = bm(global_orient=p['global_orient'], body_pose=torch.zeros(B, 63, device=device), transl=p['transl'], betas=p['betas'],
                 left_hand_pose=p['left_hand_pose'], right_hand_pose=p['right_hand_pose'])
    n = B if n is None else n                                 # frames of the window that are rendered
    verts, j, B = out.vertices[:n].contiguous(), out.joints[:n, :25], n
    c = PROX_RENDER
    joints2d = torch.stack([c['fx'] * j[..., 0] / j[..., 2] + c['cx'], c['fy'] * j[..., 1] / j[..., 2] + c['cy']], -1).contiguous()
    frames = torch.randint(0, 200, (B, c['H'], c['W'], 3), dtype=torch.uint8, device=device)
    color = (255, 0, 0)
    r = BodyRenderer(bm.faces, cull_backface=False, _lib=lib)
    img, ids = r(verts, background=frames, points=joints2d, point_radius=2, point_color=color, return_face_ids=True)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (B, c['H'], c['W'], 3) and img.device == verts.device
    cover = float((ids >= 0).float().mean())
    jn = joints2d.cpu().numpy()
    x, y = np.trunc(jn[..., 0]).astype(np.int64), np.trunc(jn[..., 1]).astype(np.int64)
    inside = np.isfinite(jn).all(-1) & (x >= 0) & (x < c['W']) & (y >= 0) & (y < c['H'])
    im = img.cpu().numpy()
    bi = np.nonzero(inside)
    hit = (im[bi[0], y[inside], x[inside]] == np.asarray(color, np.uint8)).all(-1)
    print(f'hand-over: [{B}, {c["H"]}, {c["W"]}, 3] image, body covers {cover:.3f}, joints inside the image {int(inside.sum())} of {inside.size}, '
          f'in colour {int(hit.sum())}')
    assert 0.01 < cover < 0.60
    assert inside.sum() > 0 and hit.all()
