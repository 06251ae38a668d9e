"""Cases and yardsticks for lemo_amd.scene.build_scene_sdf (csrc/scene_sdf_kernels.hip), shared by tests/test_scene_sdf_emu.py (host
emulator) and tests/test_scene_sdf_gpu.py (MI355X).  The program that made PROX's <scene>_sdf.npy was never published, so there is
nothing to run against: the yardstick is a float64 numpy restatement of the definition the kernel file states, written for these
tests, with its own normal tables (``tables64``: plain loops over faces and dictionaries, nothing shared with
``lemo_amd.scene.mesh_normal_tables``).

Per voxel centre p and valid triangle t the yardstick gives the distance d_t (Ericson's closest point by Voronoi region), the sign
s_t of (p - c_t) . n_t for the pseudonormal n_t of the feature c_t lies on, and the margin m_t = |(p - c_t) . n_t / |n_t||.  With
d* = min d_t the kernel must satisfy
    |d - d*| <= DIST_TOL, and
    its sign lies in {s_t : d_t <= d* + EPS} plus the opposite sign for those t with m_t < EPS.
A voxel is EXCUSED iff that set holds both signs.  On the float64 yardstick alone every case has at most 1 % excused voxels and at
least 5 % negative ones (asserted in a test of its own).  Brute force, grid (every side tried) and repeated runs are held to equality
on every bit, the nearest-face volume included, with no excuse list.

DIST_TOL = 4 x the largest |d32 - d64| of the SAME restatement evaluated in unfused float32 numpy (``yardstick(..., dt=float32)``) over
every case a test holds against the yardstick (``yard_cases()``).  ``measure()`` prints it: measured 2.23e-7 m (coordinates up to
3.4 m, whose ulp is 2.4e-7 m), so DIST_TOL = 8.9e-7 m.
EPS by selfpen_common.measure_eps's method: the smallest power of two for which the float32 restatement's sign disagrees with the
float64 one only on excused voxels, x 4.  Measured: NO disagreement at all on these cases, down to the floor of the search, 2^-30.  A
measurement that finds nothing cannot set the margin, so it comes from the number format: (p - c) . n is a sum of three products of
differences of fp32 coordinates of size up to 4 m; p - c carries about four roundings of 2^-24 x 4 m = 2^-20 m each way through the
closest point, 2^-18 m in all, and |n| <= 1 after normalisation: 2^-17 with a factor two in hand.  EPS = 4 x 2^-17 = 2^-15 m (3.1e-5 m), the
margin scan_common and selfpen_common give their suites.  The same EPS widens the set of near-winners.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd import scene as SCN
from lemo_amd.scene import SceneSdf, build_scene_sdf, load_prox_sdf, prepare_scene_mesh, sdf_sample
from scan_common import dev, host, icosphere, rot, torus

F32, F64 = np.float32, np.float64
DIST32_MEASURED = 2.23e-7
DIST_TOL = 4 * DIST32_MEASURED
EPS_DERIVED = 2.0 ** -17
EPS = 4 * EPS_DERIVED
EXCUSE_CAP = 0.01
MIN_NEGATIVE = 0.05
CHUNK = SCN.SDF_LDS_CHUNK

BOX_HALF = np.array([0.5, 0.4, 0.6])
BOX_ROT = rot([0.3, 1.0, 0.2], 0.37)
BOX_CENTRE = np.array([0.213, -0.147, 1.021])
BOX_FACES = np.array([[0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6]],
                     np.int64)


# ------------------------------------------------------------------------------------------------------------ meshes
def unit_box():
    """corners (+-1)^3 indexed x + 2 y + 4 z, twelve outward triangles (each face split by a coplanar diagonal)"""
    v = np.array([[(i & 1) * 2 - 1, ((i >> 1) & 1) * 2 - 1, ((i >> 2) & 1) * 2 - 1] for i in range(8)], F64)
    return v, BOX_FACES.copy()


def sheet(origin, u, v, nu, nv):
    """(nu + 1)(nv + 1) vertices origin + i u / nu + j v / nv, 2 nu nv triangles with normal u x v; open (boundary edges all round)"""
    origin, u, v = (np.asarray(x, F64) for x in (origin, u, v))
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    pts = origin + i.reshape(-1, 1) * u / nu + j.reshape(-1, 1) * v / nv
    idx = lambda a, b: a * (nv + 1) + b
    f = []
    for a in range(nu):
        for b in range(nv):
            f += [(idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)), (idx(a, b), idx(a + 1, b + 1), idx(a, b + 1))]
    return pts, np.array(f, np.int64)


def join(parts):
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + n); n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def open_room():
    """a floor, a wall, a table top (closed thin box) and two small sheets facing each other: boundary edges, single-sided surfaces,
    large empty space; rotated and moved off every lattice"""
    bv, bf = unit_box()
    parts = [sheet([-1.2, -1.0, 0.0], [2.4, 0, 0], [0, 2.0, 0], 5, 4),            # floor, normal +z
             sheet([-1.2, -1.0, 0.0], [0, 2.0, 0], [0, 0, 1.6], 4, 3),            # wall at x = -1.2, normal +x (into the room)
             (bv * np.array([0.4, 0.25, 0.02]) + np.array([0.3, 0.2, 0.7]), bf),  # table top
             sheet([0.2, -0.3, 0.9], [0.5, 0, 0], [0, 0, 0.5], 3, 3),             # normal -y ...
             sheet([0.2, -0.5, 0.9], [0, 0, 0.5], [0.5, 0, 0], 3, 3)]             # ... facing one with normal +y
    v, f = join(parts)
    return v @ rot([0.2, -0.1, 1.0], 0.23).T + np.array([0.371, 0.153, 0.097]), f


@functools.lru_cache(maxsize=None)
def sdf_case(name):
    """-> (verts float32 [V, 3], faces int64 [F, 3], dims (D, H, W)); the box is the padded default (``case_box``)"""
    if name == 'box':
        v, f = unit_box()
        v, dims = (v * BOX_HALF) @ BOX_ROT.T + BOX_CENTRE, (19, 17, 23)
    elif name == 'icosphere':
        v, f = icosphere(2)
        v, dims = v * 0.8 + np.array([-0.113, 0.247, 2.021]), (24, 21, 26)
    elif name == 'torus':
        v, f = torus()
        v, dims = v @ rot([1.0, 0.3, 0.1], 1.05).T + np.array([-0.103, 0.097, 2.513]), (25, 22, 27)
    elif name == 'room':
        (v, f), dims = open_room(), (26, 23, 21)
    else:
        raise KeyError(name)
    v = v.astype(F32)
    v.setflags(write=False)
    return v, f, dims


CASES = ('box', 'icosphere', 'torus', 'room')


def case_box(name):
    """explicit bounds for the yardstick runs: the padded default of build_scene_sdf, restated"""
    v, f, dims = sdf_case(name)
    used = v[f.reshape(-1)].astype(F64)
    return (used.min(0) - 0.25).astype(F32), (used.max(0) + 0.25).astype(F32)


def centres64(gmin, gmax, dims):
    ax = [F64(gmin[a]) + (np.arange(dims[a]) + 0.5) * (F64(gmax[a]) - F64(gmin[a])) / dims[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------ float64 yardstick
def valid64(v, f):
    V = len(v)
    ok = np.all((f >= 0) & (f < V), axis=1)
    c = v.astype(F64)[np.where(ok[:, None], f, 0)]
    with np.errstate(all='ignore'):
        n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ok &= np.all(np.isfinite(c.reshape(len(f), 9)), axis=1) & (np.sum(n * n, axis=1) > 0)
    return ok


def tables64(v, f):
    """the tests' own normal tables -> N [F, 7, 3]: face normal, three edge pseudonormals, three vertex pseudonormals per face"""
    v = v.astype(F64)
    ok = valid64(v, f)
    unit, edge_sum, vert_sum = {}, {}, {}
    for t in np.nonzero(ok)[0]:
        a, b, c = (v[i] for i in f[t])
        n = np.cross(b - a, c - a)
        unit[t] = n / np.linalg.norm(n)
        for k in range(3):
            i, j, l = int(f[t][k]), int(f[t][(k + 1) % 3]), int(f[t][(k + 2) % 3])
            key = (min(i, j), max(i, j))
            edge_sum[key] = edge_sum.get(key, 0) + unit[t]
            e1, e2 = v[j] - v[i], v[l] - v[i]
            ang = np.arccos(np.clip(e1 @ e2 / (np.linalg.norm(e1) * np.linalg.norm(e2)), -1, 1))
            vert_sum[i] = vert_sum.get(i, 0) + ang * unit[t]
    N = np.zeros((len(f), 7, 3))
    for t in unit:
        N[t, 0] = unit[t]
        for k in range(3):
            i, j = int(f[t][k]), int(f[t][(k + 1) % 3])
            N[t, 1 + k] = edge_sum[(min(i, j), max(i, j))]
            N[t, 4 + k] = vert_sum[i]
    return N, ok


def closest(p, a, b, c, dt):
    """Ericson's closest point, p [N, 1, 3] against triangles [1, T, 3] in dtype ``dt`` (plain numpy arithmetic: unfused) ->
    (d2 [N, T], q = p - closest [N, T, 3], feature [N, T]: 0 face, 1 .. 3 edge ab / bc / ca, 4 .. 6 vertex a / b / c)"""
    p, a, b, c = (x.astype(dt) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    bp, cp = ap - ab, ap - ac
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    feat = np.select(conds, [4, 5, 1, 6, 3, 2], 0)
    ns = np.select(conds, [zero, one, d1, zero, zero, e56], vb)
    nt = np.select(conds, [zero, zero, zero, one, d2, e43], vc)
    dn = np.select(conds, [one, one, d1 - d3, one, d2 - d6, e43 + e56], va + vb + vc)
    with np.errstate(all='ignore'):
        s, t = ns / dn, nt / dn
    q = ap - s[..., None] * ab - t[..., None] * ac
    return dot(q, q), q, feat


class Yard:
    """per-voxel summary of the yardstick: d* , the winner's face and sign, the acceptable signs"""
    def __init__(self, d, face, neg, may_neg, may_pos):
        self.d, self.face, self.neg, self.may_neg, self.may_pos = d, face, neg, may_neg, may_pos
        self.excused = may_neg & may_pos


def yardstick(v, f, gmin, gmax, dims, dt=F64, eps=EPS, block=1024):
    """the restatement in dtype ``dt`` (tables rounded to it); the acceptable sets are only meaningful for float64"""
    N7, ok = tables64(v, f)
    tid = np.nonzero(ok)[0]
    P = centres64(gmin, gmax, dims)
    n = len(P)
    if len(tid) == 0:
        z = np.zeros(n, bool)
        return Yard(np.full(n, np.inf), np.full(n, -1), z, z, ~z)
    vv = v.astype(F64)
    A, B, C = (vv[f[tid, k]][None] for k in range(3))
    N7 = N7[tid].astype(dt)
    unit7 = N7.astype(F64) / np.maximum(np.linalg.norm(N7.astype(F64), axis=-1, keepdims=True), 1e-300)
    out = [[] for _ in range(5)]
    for s in range(0, n, block):
        p = P[s:s + block, None, :]
        d2, q, feat = closest(p, A, B, C, dt)
        d = np.sqrt(d2.astype(F64))
        nrm = np.take_along_axis(np.broadcast_to(N7[None], (len(p),) + N7.shape), feat[..., None, None].repeat(3, -1), axis=2)[:, :, 0]
        sd = (q[..., 0] * nrm[..., 0] + q[..., 1] * nrm[..., 1]) + q[..., 2] * nrm[..., 2]
        neg = sd < 0
        un = np.take_along_axis(np.broadcast_to(unit7[None], (len(p),) + unit7.shape), feat[..., None, None].repeat(3, -1), axis=2)[:, :, 0]
        m = np.abs(np.sum(q.astype(F64) * un, axis=-1))
        w = np.argmin(d2, axis=1)                                                      # first minimum: the lowest face index
        rows = np.arange(len(p))
        dstar = d[rows, w]
        near = d <= dstar[:, None] + eps
        out[0].append(dstar); out[1].append(tid[w]); out[2].append(neg[rows, w])
        out[3].append(np.any(near & (neg | (m < eps)), axis=1)); out[4].append(np.any(near & (~neg | (m < eps)), axis=1))
    return Yard(*[np.concatenate(o) for o in out])


@functools.lru_cache(maxsize=None)
def reference(name):
    v, f, dims = sdf_case(name)
    gmin, gmax = case_box(name)
    return yardstick(v, f, gmin, gmax, dims)


def yard_cases():
    """every (verts, faces, grid_min, grid_max, dims) that a test holds against the yardstick"""
    for name in CASES:
        v, f, dims = sdf_case(name)
        yield (name, v, f) + case_box(name) + (dims,)
    for name in EDGE_CASES:
        v, f, dims, gmin, gmax = edge_case(name)
        yield name, v, f, gmin, gmax, dims


def measure():
    """the docstring's two measurements over yard_cases() -> (largest |d32 - d64|, smallest power of two that excuses every float32
    sign error, or None)"""
    worst, runs = 0.0, []
    for name, v, f, gmin, gmax, dims in yard_cases():
        y32, y64 = yardstick(v, f, gmin, gmax, dims, dt=F32), yardstick(v, f, gmin, gmax, dims)
        err = float(np.max(np.abs(y32.d - y64.d)))
        print(f'{name}: |d32 - d64| <= {err:.3g}, sign disagreements {int((y32.neg != y64.neg).sum())}')
        worst = max(worst, err)
        runs.append((v, f, gmin, gmax, dims, y32.neg))
    for e in range(30, 5, -1):
        ok = True
        for v, f, gmin, gmax, dims, neg32 in runs:
            y = yardstick(v, f, gmin, gmax, dims, eps=2.0 ** -e)
            ok = ok and not np.any((neg32 != y.neg) & ~y.excused)
        if ok:
            return worst, 2.0 ** -e
    return worst, None


def box_closed_form(P):
    q = np.abs((P - BOX_CENTRE) @ BOX_ROT) - BOX_HALF
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


# ------------------------------------------------------------------------------------------------------------ checks
def _build(lib, device, v, f, dims, gmin=None, gmax=None, **kw):
    return build_scene_sdf(dev(v, device, F32), f, dim=dims, grid_min=gmin, grid_max=gmax, return_nearest=True, _lib=lib, **kw)


def check_modes_identical(lib, device, v, f, dims, gmin=None, gmax=None, grids=(2, 5, None)):
    """brute force twice, grid at several sides, auto, faces as a device tensor, a prepared mesh: the same bits"""
    base = _build(lib, device, v, f, dims, gmin, gmax, mode='brute')
    again = _build(lib, device, v, f, dims, gmin, gmax, mode='brute')
    assert torch.equal(base.sdf.view(torch.int32), again.sdf.view(torch.int32)) and torch.equal(base.nearest, again.nearest)
    for extra in [dict(mode='grid', grid=g) for g in grids] + [dict(mode='grid', grid=grids[0]), dict(mode='auto')]:
        got = _build(lib, device, v, f, dims, gmin, gmax, **extra)
        same = torch.equal(got.sdf.view(torch.int32), base.sdf.view(torch.int32))
        assert same, f'{extra}: {int((got.sdf.view(torch.int32) != base.sdf.view(torch.int32)).sum())} voxels differ from brute force'
        assert torch.equal(got.nearest, base.nearest), f'{extra}: the nearest-face volume differs from brute force'
        assert np.array_equal(got.grid_min, base.grid_min) and np.array_equal(got.grid_max, base.grid_max)
    mesh = prepare_scene_mesh(dev(v, device, F32), dev(f, device, np.int32), _lib=lib)
    got = build_scene_sdf(mesh, dim=dims, grid_min=base.grid_min, grid_max=base.grid_max, mode='grid', grid=7, return_nearest=True, _lib=lib)
    assert torch.equal(got.sdf.view(torch.int32), base.sdf.view(torch.int32)) and torch.equal(got.nearest, base.nearest)
    return base


def compare(S, y, what):
    """the kernel's volume against a Yard"""
    sdf = host(S.sdf).reshape(-1).astype(F64)
    err = float(np.max(np.abs(np.abs(sdf) - y.d)))
    neg = sdf < 0
    bad = (neg & ~y.may_neg) | (~neg & ~y.may_pos)
    print(f'{what}: {len(sdf)} voxels, {int(neg.sum())} negative, max |d - d*| = {err:.3g} (tol {DIST_TOL:.3g}), excused {int(y.excused.sum())}, '
          f'sign outside the set {int(bad.sum())}')
    assert err <= DIST_TOL, f'{what}: distance off by {err}'
    assert not bad.any(), f'{what}: {int(bad.sum())} voxels with a sign outside the acceptable set'
    # the winner is a nearest triangle, up to the distance tolerance
    return sdf


def check_case(lib, device, name):
    v, f, dims = sdf_case(name)
    S = check_modes_identical(lib, device, v, f, dims)                                # the padded default box
    gmin, gmax = case_box(name)
    assert np.array_equal(S.grid_min, gmin) and np.array_equal(S.grid_max, gmax), 'the default box is the valid triangles\' box + padding'
    assert S.dims == dims and S.sdf.dtype == torch.float32 and S.nearest.dtype == torch.int32
    y = reference(name)
    compare(S, y, name)
    near = host(S.nearest).reshape(-1)
    assert near.min() >= 0 and near.max() < len(f)
    if name == 'box':
        sdf = host(S.sdf).reshape(-1).astype(F64)
        cf = box_closed_form(centres64(gmin, gmax, dims))
        err = float(np.max(np.abs(sdf - cf)))
        print(f'box against its closed form: {err:.3g}')
        assert err <= DIST_TOL
        away = np.abs(cf) > EPS
        assert np.array_equal(sdf[away] < 0, cf[away] < 0)


def check_yardstick_conditions():
    for name in CASES:
        y = reference(name)
        n = len(y.d)
        print(f'{name}: {n} voxels, excused {int(y.excused.sum())}, negative {int(y.neg.sum())}')
        assert y.excused.sum() <= EXCUSE_CAP * n, (name, int(y.excused.sum()), n)
        assert y.neg.sum() >= MIN_NEGATIVE * n, (name, int(y.neg.sum()), n)
    v, f, dims = sdf_case('box')
    y = reference('box')
    cf = box_closed_form(centres64(*case_box('box'), dims))
    assert np.max(np.abs(np.where(y.neg, -y.d, y.d) - cf)) < 1e-7                      # fp32 corners: the rotation is rounded


def edge_sheet():
    """a 16 x 8 sheet: 2 x 16 x 8 = 256 triangles = one LDS chunk"""
    v, f = sheet([-0.8, -0.4, 0.0], [1.6, 0, 0], [0, 0.8, 0], 16, 8)
    assert len(f) == CHUNK
    return (v @ rot([0.4, 1.0, -0.3], 0.31).T + np.array([0.117, -0.059, 1.213])).astype(F32), f


E_MIN, E_MAX = np.array([-1.1, -0.9, 0.55], F32), np.array([1.3, 0.7, 1.85], F32)
ONE_V = np.array([[0.1, -0.2, 1.0], [0.9, 0.1, 1.1], [0.2, 0.5, 1.4]], F32)
ONE_F = np.array([[0, 1, 2]])


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """the meshes of check_edge_rules that are held against the yardstick -> (verts, faces, dims, grid_min, grid_max)"""
    v, f = edge_sheet()
    f257 = np.concatenate([f, f[5:6]])             # F = one more than the chunk; the extra triangle duplicates face 5
    if name == 'sheet + duplicate':
        return v, f257, (11, 1, 13), E_MIN, E_MAX  # a side of 1, sides that are no multiple of the brick
    if name == 'F = 1':
        return ONE_V, ONE_F, (5, 9, 7), E_MIN, E_MAX
    if name == 'sheet, small box':                 # a box that cuts through the mesh and leaves most of it outside
        return v, f257, (9, 10, 7), np.array([0.2, -0.3, 1.0], F32), np.array([0.5, 0.1, 1.6], F32)
    if name == 'torus, distant box':               # all of the mesh outside the box
        tv, tf, _ = sdf_case('torus')
        return tv, tf, (7, 5, 9), np.array([1.2, 0.9, 2.4], F32), np.array([1.9, 1.5, 3.3], F32)
    raise KeyError(name)


EDGE_CASES = ('sheet + duplicate', 'F = 1', 'sheet, small box', 'torus, distant box')


def check_edge_rules(lib, device):
    runs = {}
    for name in EDGE_CASES:
        v, f, dims, gmin, gmax = edge_case(name)
        runs[name] = check_modes_identical(lib, device, v, f, dims, gmin, gmax)
        compare(runs[name], yardstick(v, f, gmin, gmax, dims), name)
    v, f, dims, _, _ = edge_case('sheet + duplicate')
    near = host(runs['sheet + duplicate'].nearest)
    assert (near == 5).any() and not (near == CHUNK).any(), 'of two equal triangles the lower index wins'
    S256 = check_modes_identical(lib, device, v, f[:CHUNK], dims, E_MIN, E_MAX)
    assert torch.equal(S256.nearest, runs['sheet + duplicate'].nearest)
    S1 = runs['F = 1']
    assert int(host(S1.nearest).max()) == 0
    # a zero-area triangle and one with a NaN corner next to it are ignored: the same volume, and the same default box
    junk_v = np.concatenate([ONE_V, np.array([[0.5, 0.5, 0.9], [np.nan, 0.0, 1.0], [30.0, 30.0, 30.0]], F32)])
    junk_f = np.array([[3, 3, 3], [0, 1, 1], [0, 1, 2], [0, 4, 2], [5, 5, 5]])
    Sj = check_modes_identical(lib, device, junk_v, junk_f, (5, 9, 7), E_MIN, E_MAX)
    assert torch.equal(Sj.sdf.view(torch.int32), S1.sdf.view(torch.int32)) and set(np.unique(host(Sj.nearest))) == {2}
    Sd, S1d = _build(lib, device, junk_v, junk_f, 6), _build(lib, device, ONE_V, ONE_F, 6)
    assert np.array_equal(Sd.grid_min, S1d.grid_min) and np.array_equal(Sd.grid_max, S1d.grid_max)
    assert np.allclose(S1d.grid_min, ONE_V.min(0) - 0.25) and np.allclose(S1d.grid_max, ONE_V.max(0) + 0.25)
    # no valid triangle: +inf, nearest -1; and the default box has nothing to stand on
    none_f = np.array([[0, 1, 1], [0, 4, 2]])
    for mode in ('brute', 'grid', 'auto'):
        Sn = _build(lib, device, junk_v, none_f, (3, 4, 9), E_MIN, E_MAX, mode=mode)
        assert bool(torch.isinf(Sn.sdf).all()) and bool((Sn.sdf > 0).all()) and bool((Sn.nearest == -1).all())
    with pytest.raises(ValueError):
        _build(lib, device, junk_v, none_f, 4)


def check_sampler(lib, device):
    """sdf_sample at the centres returns the volume, bit for bit.  The box and the dims are powers of two (D != H != W), so the
    sampler's own float32 coordinate arithmetic ((p - min) * 2 / extent - 1, then * dim) is exact and the weights are exactly 0; with
    arbitrary bounds that arithmetic rounds, and the sampler blends in 1e-7 of a neighbour."""
    v, f, _ = sdf_case('room')                                                         # asymmetric
    gmin, gmax = np.array([-1.0, -1.5, -0.5], F32), np.array([1.0, 2.5, 1.5], F32)
    S = build_scene_sdf(dev(v, device, F32), f, dim=(8, 32, 16), grid_min=gmin, grid_max=gmax, _lib=lib)
    c = S.centres()
    assert tuple(c.shape) == (8, 32, 16, 3)
    assert np.array_equal(host(c).reshape(-1, 3).astype(F64), centres64(gmin, gmax, (8, 32, 16)))
    got = sdf_sample(c, S.sdf, S.grid_min, S.grid_max, _lib=lib)
    assert torch.equal(got.view(torch.int32), S.sdf.view(torch.int32))
    swapped = sdf_sample(c[..., [2, 1, 0]], S.sdf, S.grid_min, S.grid_max, _lib=lib)
    assert not torch.equal(swapped, S.sdf), 'an x / z swap must not pass'
    kw = S.fitter_kwargs()
    assert set(kw) == {'sdf', 'grid_min', 'grid_max'} and kw['sdf'] is S.sdf and np.array_equal(kw['grid_min'], gmin)


def check_files(lib, device, tmp_path):
    v, f, _ = sdf_case('room')
    S = build_scene_sdf(dev(v, device, F32), f, dim=12, _lib=lib)
    S.save_prox(str(tmp_path), 'MyRoom')
    # fit_temp_loadprox_slide.py:287-294, restated
    with open(os.path.join(str(tmp_path), 'MyRoom.json')) as fh:
        sdf_data = json.load(fh)
    grid_min, grid_max, grid_dim = np.array(sdf_data['min'], F32), np.array(sdf_data['max'], F32), sdf_data['dim']
    sdf = np.load(os.path.join(str(tmp_path), 'MyRoom_sdf.npy')).reshape(grid_dim, grid_dim, grid_dim)
    assert grid_dim == 12 and sdf.dtype == F32 and np.array_equal(sdf, host(S.sdf))
    assert np.array_equal(grid_min, S.grid_min) and np.array_equal(grid_max, S.grid_max)
    L = load_prox_sdf(str(tmp_path), 'MyRoom', device)
    assert torch.equal(L.sdf.view(torch.int32), S.sdf.view(torch.int32)) and L.sdf.device == S.sdf.device and L.dims == (12, 12, 12)
    assert np.array_equal(L.grid_min, S.grid_min) and np.array_equal(L.grid_max, S.grid_max) and L.grid_min.dtype == F32
    with pytest.raises(ValueError):
        build_scene_sdf(dev(v, device, F32), f, dim=(4, 5, 4), _lib=lib).save_prox(str(tmp_path), 'Flat')


def check_graph(lib, device):
    """GPU only: a captured and replayed build equals the eager one, bit for bit"""
    v, f, dims = sdf_case('room')
    gmin, gmax = case_box('room')
    mesh = prepare_scene_mesh(dev(v, device, F32), f, _lib=lib)
    for mode in ('grid', 'brute'):
        eager = build_scene_sdf(mesh, dim=dims, grid_min=gmin, grid_max=gmax, mode=mode, return_nearest=True, _lib=lib)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                cap = build_scene_sdf(mesh, dim=dims, grid_min=gmin, grid_max=gmax, mode=mode, return_nearest=True, _lib=lib)
            for _ in range(2):
                cap.sdf.fill_(7.0); cap.nearest.fill_(-7)
                graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.sdf.view(torch.int32), eager.sdf.view(torch.int32)) and torch.equal(cap.nearest, eager.nearest), mode


def check_validation(lib, device, monkeypatch):
    launched = []
    monkeypatch.setattr(lib, 'scene_sdf_build', lambda *a: launched.append('scene_sdf_build') or 0)
    v, f, dims = sdf_case('box')
    V = len(v)
    vt = dev(v, device, F32)
    E = (ValueError, _hip.LemoHipError)
    big_f = np.zeros(((1 << 22) + 1, 3), np.int32)
    for kw in (dict(vertices=vt.double()), dict(vertices=vt[:, :2]), dict(vertices=vt[None]), dict(vertices=v), dict(faces=f.astype(F64)),
               dict(faces=f[:, :2]), dict(faces=np.concatenate([f, [[0, 1, V]]])), dict(faces=np.concatenate([f, [[0, -1, 2]]])),
               dict(faces=dev(f, device, np.int64)), dict(faces=None), dict(faces=big_f), dict(mode='tree'), dict(grid=1), dict(grid=33), dict(grid=0),
               dict(dim=0), dict(dim=1025), dict(dim=(1024, 1024, 512)), dict(dim=(4, 4)), dict(dim=2.5), dict(dim=(4, 4, 2.0)),
               dict(grid_min=[0, 0, 0]), dict(grid_max=[1, 1, 1]), dict(grid_min=[0, 0, 0], grid_max=[1, 1, float('nan')]),
               dict(grid_min=[0, 0, 0], grid_max=[1, 1, float('inf')]), dict(grid_min=[0, 0, 0], grid_max=[1, 0, 1]),
               dict(grid_min=[0, 0, 0], grid_max=[1, -1, 1]), dict(grid_min=[0, 0], grid_max=[1, 1]),
               dict(grid_min=[1.0, 0, 0], grid_max=[1.0 + 1e-9, 1, 1]),                # empty once rounded to float32
               dict(grid_min=[-1e39, 0, 0], grid_max=[1, 1, 1]), dict(padding=-0.1), dict(padding=float('nan'))):
        args = dict(vertices=vt, faces=f, dim=8, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            build_scene_sdf(**args)
    if device.type != 'cpu':
        with pytest.raises(E):
            build_scene_sdf(vt.cpu(), f, dim=8, _lib=lib)
    mesh = prepare_scene_mesh(vt, f, _lib=lib)
    with pytest.raises(E):
        build_scene_sdf(mesh, f, dim=8, _lib=lib)
    assert launched == []
    assert isinstance(build_scene_sdf(mesh, dim=8, _lib=lib), SceneSdf) and launched == ['scene_sdf_build']
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    import ctypes as C
    S, A = 10001, 10002
    wsb = lib.scene_sdf_ws_bytes
    assert wsb(0, 4, 4, 4, 0, 0) == -1 and wsb(1, 0, 4, 4, 0, 0) == -1 and wsb(1, 4, 1025, 4, 0, 0) == -1 and wsb(1, 1024, 1024, 512, 1, 0) == -1
    assert wsb((1 << 22) + 1, 4, 4, 4, 1, 0) == -1 and wsb(1, 4, 4, 4, 3, 0) == -1 and wsb(1, 4, 4, 4, 2, 1) == -1 and wsb(1, 4, 4, 4, 2, 33) == -1
    assert wsb(100, 4, 4, 4, 1, 0) == 0 and wsb(100, 4, 4, 4, 2, 3) == 4 * (16 + 5 * 27 + 1 + 10 * 100) and wsb(100, 64, 8, 8, 2, 0) == wsb(100, 8, 8, 8, 2, 8)
    g0, g1 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    gn = (C.c_float * 3)(0, float('nan'), 0)

    def bd(V=3, F=1, D=4, H=4, W=4, mode=1, grid=0, x=1, out=1, lo=g0, hi=g1, ws=1, wsb=1 << 20, tab=1):
        return lib.scene_sdf_build(x, V, 1, F, tab, 1, 1, lo, hi, D, H, W, mode, grid, out, None, ws, wsb, None)
    assert bd(V=0) == S and bd(F=0) == S and bd(D=0) == S and bd(W=1025) == S and bd(D=1024, H=1024, W=512) == S and bd(F=(1 << 22) + 1) == S
    assert bd(mode=3) == A and bd(mode=-1) == A and bd(grid=1) == A and bd(grid=33) == A and bd(x=None) == A and bd(out=None) == A and bd(tab=None) == A
    assert bd(lo=None) == A and bd(lo=g1, hi=g0) == A and bd(lo=g0, hi=g0) == A and bd(hi=gn) == A
    assert bd(mode=2, ws=None) == A and bd(mode=2, wsb=64) == A
