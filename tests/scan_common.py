"""Cases and yardsticks for lemo_amd.scan (csrc/visibility_kernels.hip, lemo_chamfer_masked_forward), shared by tests/test_scan_emu.py
(host emulator) and tests/test_scan_gpu.py (MI355X).  The yardsticks are numpy / float64 torch restatements written for these tests.

Visibility.  The kernels evaluate Moeller-Trumbore with the camera as the origin, in fp32, without a division (see the kernel file).
The yardstick is the textbook form in float64 from the other end of the segment: origin o = p + min_dist dir, direction c - o,
u, v, t by division.  The two agree wherever the answer does not hang on a rounding: a vertex is EXCUSED iff the float64 answer
differs between a strict evaluation (u, v >= eps, u + v <= 1 - eps, eps <= t <= 1 - eps) and a loose one (the same bounds with
-eps); everywhere else the kernel must equal the float64 answer.  eps is measured, not guessed: ``measure_eps`` looks for the
smallest power of two for which a float32 numpy restatement of the kernel's own formulation (``hits32``: unfused, so it rounds more
often than the kernel) disagrees with float64 only on excused vertices over all cases below.  Measured: NO disagreement at all on
these cases, down to the floor of the search, 2^-30.  A measurement that finds nothing cannot set the margin, so the value comes from
the number format instead: u and v carry an error of about 2^-22 |P| / |e| (the kernel file's error estimate of an edge function over
det = |w| |e1| |e2|), which is 2^-17 at the |P| / |e| = 3 m / 0.1 m of these meshes; eps = 4 x that = 2^-15, the margin the occlusion
suite gives its float32 restatement.  It stays a factor 10 below the 3.3e-4 by which a vertex's own triangles miss the segment
(min_dist / |w| at 3 m), so they excuse nothing.  The excused vertices are capped at 1 % of each case's vertices (a condition on the
cases, asserted: the float64 yardstick alone stays within it for these poses).
Brute force and binned are held to equality on every bit, with no excuse list.

Masked nearest neighbours: the derivations of tests/chamfer_common.py's docstring, among the VALID targets: forward
``|dist - d64[idx]| <= 6 * 2^-24 * d64[idx]``, ``d64[idx] <= (1 + 12 * 2^-24) min over valid d64``; lattice inputs exact with the lowest
valid index; backward ``4 K 2^-24 sum|terms|``.

Terms: 1e-5 relative for the loss scalars and their gradients (the project's loss-scalar tolerance), against a float64
torch restatement of fitting_temp_slide.py:650-670 that is handed the kernel's own visibility.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd import chamfer as CH
from lemo_amd import scan as SC
from lemo_amd.chamfer import chamfer_distance
from lemo_amd.scan import gmof, masked_nearest, scan_terms, vertex_visibility

F32, F64 = np.float32, np.float64
EPS24 = 2.0 ** -24
VIS_EPS_MEASURED = 2.0 ** -17
VIS_EPS = 4 * VIS_EPS_MEASURED
EXCUSE_CAP = 0.01
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_Q, _C, _L = CH.QUERIES_PER_WORKGROUP, CH.LDS_CHUNK, CH.SPLIT_LENGTH


def dev(a, device, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(device)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def icosphere(level=3):
    """642 vertices / 1280 faces at level 3; unit radius, outward winding"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, F64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, F64), np.array(f, np.int64)


def torus(nu=32, nv=16, R=0.5, r=0.2):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, np.int64)


def rot(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


SHEET_TRI = np.array([[-0.34, -0.295, 2.0], [0.326, -0.268, 2.0], [0.031, 0.329, 2.0]])      # clear of every projected sheet point


def sheet_mesh():
    """one large triangle at z = 2 in front of a 20 x 20 point sheet at z = 3 (the sheet has no faces)"""
    g = np.linspace(-0.5, 0.5, 20)
    x, y = np.meshgrid(g, g, indexing='ij')
    sheet = np.stack([x.ravel(), y.ravel(), np.full(x.size, 3.0)], -1)
    return np.concatenate([sheet, SHEET_TRI]), np.array([[400, 401, 402]], np.int64)


def sheet_closed_form():
    """a sheet point (x, y, 3) is hidden iff (2 x / 3, 2 y / 3) lies inside the triangle; -> (vis [403], smallest |edge function|)"""
    v, _ = sheet_mesh()
    p = v[:400, :2] * (2.0 / 3.0)
    a, b, c = SHEET_TRI[:, :2]
    e = lambda s, t: (t[0] - s[0]) * (p[:, 1] - s[1]) - (t[1] - s[1]) * (p[:, 0] - s[0])
    e0, e1, e2 = e(a, b), e(b, c), e(c, a)
    inside = ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0))
    margin = np.min(np.abs(np.stack([e0, e1, e2])))
    return np.concatenate([~inside, np.ones(3, bool)]).astype(np.uint8), float(margin)


@functools.lru_cache(maxsize=None)
def vis_case(name, B):
    """-> (verts float32 [B, V, 3], faces int64 [F, 3], cam float32 [3] or None); the frames are rigid moves of one another"""
    sv, sf = icosphere()
    cam = None
    if name == 'sphere':
        v, f = sv * 0.5 + np.array([0.1, -0.05, 3.0]), sf
    elif name == 'two_spheres':
        v = np.concatenate([sv * 0.3 + np.array([0.12, 0.05, 2.0]), (sv @ rot([0.3, 1.0, 0.2], 0.37).T) * 0.5 + np.array([0.031, -0.017, 3.6])])
        f = np.concatenate([sf, sf + len(sv)])
    elif name == 'torus':
        tv, f = torus()
        v = tv @ rot([1.0, 0.3, 0.1], 1.05).T + np.array([-0.1, 0.1, 2.5])
    elif name == 'sheet':
        v, f = sheet_mesh()
    elif name == 'sphere_cam':
        v, f, cam = sv * 0.5 + np.array([0.1, -0.05, 3.0]) + np.array([0.3, -0.2, 0.5]), sf, np.array([0.3, -0.2, 0.5], F32)
    else:
        raise KeyError(name)
    frames = [v]
    c0 = np.zeros(3) if cam is None else cam.astype(F64)
    for k in range(1, B):                                         # a turn about the viewing axis and a small shift, about the camera
        frames.append((v - c0) @ rot([0.05 * k, 0.02, 1.0], 0.4 * k).T + np.array([0.07 * k, -0.04 * k, 0.15 * k]) + c0)
    verts = np.stack(frames).astype(F32)
    verts.setflags(write=False)
    return verts, f, cam


VIS_CASES = [(n, B) for n in ('sphere', 'two_spheres', 'torus', 'sheet', 'sphere_cam') for B in (1, 3)]


# ------------------------------------------------------------------------------------------------------------ yardsticks
def _rays(v, c, min_dist, dt):
    p, c = v.astype(dt), np.asarray(c, dt)
    d = c - p
    ln = np.sqrt((d * d).sum(-1, keepdims=True))
    o = p + dt(min_dist) * d / ln
    return o, ln[:, 0] > min_dist


def hits64(v, f, c, min_dist, eps, chunk=256):
    """float64 Moeller-Trumbore from o towards c for one frame -> (visible strict, visible loose, visible plain), each bool [n]"""
    o, test = _rays(v, c, min_dist, F64)
    v64, c = v.astype(F64), np.asarray(c, F64)
    v0, e1, e2 = v64[f[:, 0]], v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]
    out = [np.ones(len(o), bool) for _ in range(3)]
    with np.errstate(all='ignore'):
        for lo in range(0, len(o), chunk):
            oo = o[lo:lo + chunk]
            D = (c - oo)[:, None, :]
            pv = np.cross(D, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo[:, None, :] - v0[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            w = (D * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            for k, m in enumerate((eps, -eps, 0.0)):
                hit = (det != 0) & (u >= m) & (w >= m) & (u + w <= 1 - m) & (t >= m) & (t <= 1 - m)
                out[k][lo:lo + chunk] = ~(hit.any(1) & test[lo:lo + chunk])
    return out


def hits32(v, f, c, min_dist):
    """the kernel's own formulation (camera origin, no division) in float32 numpy, unfused -> visible bool [V]; used to measure eps"""
    c = np.asarray(c, F32)
    p = v.astype(F32)
    d = c - p
    ln = np.sqrt(d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]))
    test = ln > F32(min_dist)
    with np.errstate(all='ignore'):
        s = F32(min_dist) / ln
        w = (p + s[:, None] * d) - c
        P = p - c
        P0, e1, e2 = P[f[:, 0]], P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]]
        nd, a, q = np.cross(e2, e1).astype(F32), np.cross(P0, e2).astype(F32), np.cross(e1, P0).astype(F32)
        tn = (P0 * nd).sum(-1, dtype=F32)
        det, U, V = w @ nd.T, w @ a.T, w @ q.T
        S = U + V
        m = ((P0[None] - w[:, None]) * nd[None]).sum(-1, dtype=F32)
        pos = (det > 0) & (U >= 0) & (V >= 0) & (S <= det) & (tn[None] >= 0) & (m <= 0)
        neg = (det < 0) & (U <= 0) & (V <= 0) & (S >= det) & (tn[None] <= 0) & (m >= 0)
    return ~((pos | neg).any(1) & test)


@functools.lru_cache(maxsize=None)
def vis_reference(name, B):
    verts, f, cam = vis_case(name, B)
    c = np.zeros(3) if cam is None else cam
    ref = [hits64(verts[b], f, c, 1e-3, VIS_EPS) for b in range(B)]
    strict, loose, plain = (np.stack([r[k] for r in ref]) for k in range(3))
    return strict, loose, plain


def measure_eps():
    """the docstring's measurement: smallest power of two for which hits32 disagrees with float64 only on excused vertices"""
    for e in range(30, 5, -1):
        eps, ok = 2.0 ** -e, True
        for name, B in VIS_CASES:
            verts, f, cam = vis_case(name, B)
            c = np.zeros(3) if cam is None else cam
            for b in range(B):
                s, l, p = hits64(verts[b], f, c, 1e-3, eps)
                ok = ok and not np.any((hits32(verts[b], f, c, 1e-3) != p) & (s == l))
        if ok:
            return eps
    return None


# ------------------------------------------------------------------------------------------------------------ visibility checks
def _vis(lib, device, verts, f, cam, **kw):
    return host(vertex_visibility(dev(verts, device), f, cam=cam, _lib=lib, **kw))


def check_visibility(lib, device, name, B):
    verts, f, cam = vis_case(name, B)
    brute = _vis(lib, device, verts, f, cam, mode='brute')
    assert brute.dtype == np.uint8 and brute.shape == verts.shape[:2] and set(np.unique(brute)) <= {0, 1}
    binned, nbig = vertex_visibility(dev(verts, device), f, cam=cam, mode='binned', return_big=True, _lib=lib)
    assert np.array_equal(brute, host(binned)), f'{name}: binned differs from brute force on {(brute != host(binned)).sum()} vertices'
    assert np.array_equal(brute, _vis(lib, device, verts, f, cam, mode='binned', grid=16)), 'grid 16 differs'
    assert np.array_equal(brute, _vis(lib, device, verts, f, cam, mode='auto')), 'auto differs'
    assert np.array_equal(brute, _vis(lib, device, verts, dev(f, device, np.int32), cam, mode='binned', grid=5))
    strict, loose, plain = vis_reference(name, B)
    excused = strict != loose
    share = excused.mean(1)
    print(f'{name} B = {B}: visible {brute.mean(1)}, excused {excused.sum(1)} of {verts.shape[1]}, big / thin triangles {host(nbig)}')
    assert np.all(share <= EXCUSE_CAP), f'{name}: {share} of the vertices are excused (cap {EXCUSE_CAP})'
    bad = (brute.astype(bool) != plain) & ~excused
    assert not bad.any(), f'{name}: {bad.sum()} vertices differ from float64 outside the excuse set'
    if name == 'sphere':
        assert np.all((brute.mean(1) > 0.30) & (brute.mean(1) < 0.60))
    if name == 'two_spheres':
        n = len(icosphere()[0])
        alone = _vis(lib, device, verts[:, n:], icosphere()[1], cam, mode='brute')
        hidden = (alone == 1) & (brute[:, n:] == 0)
        assert np.all(hidden.sum(1) >= 50) and np.all(brute[:, n:].sum(1) >= 50), (hidden.sum(1), brute[:, n:].sum(1))
    if name == 'sheet':
        want, margin = sheet_closed_form()
        assert margin > 1e-3                                      # edge functions (twice an area): no sheet point projects near an edge
        assert np.array_equal(brute[0], want) and 0 < want[:400].sum() < 400
        assert int(host(nbig)[0]) == 1                            # the one triangle took the one-workgroup-per-triangle pass


def check_fallback(lib, device):
    """one frame of three has vertices at and behind the camera plane: it takes the brute-force path inside the binned call"""
    verts, f, _ = vis_case('sphere', 3)
    verts = verts.copy()
    verts[1] = verts[1] - np.array([0.0, 0.0, 2.9], F32)          # the sphere of radius 0.5 now contains the camera plane
    assert verts[1, :, 2].min() <= 0 < verts[1, :, 2].max()
    brute = _vis(lib, device, verts, f, None, mode='brute')
    for grid in (0, 16):
        got, nbig = vertex_visibility(dev(verts, device), f, mode='binned', grid=grid, return_big=True, _lib=lib)
        assert np.array_equal(host(got), brute)
        assert int(host(nbig)[1]) == 0                            # nothing of that frame went through the bins
    near = vis_case('sphere', 1)[0].copy()
    near[0, 0] = 0.0                                              # a vertex ON the camera: |c - p| <= min_dist counts as visible
    assert _vis(lib, device, near, f, None, mode='brute')[0, 0] == 1
    assert np.array_equal(_vis(lib, device, near, f, None, mode='brute'), _vis(lib, device, near, f, None, mode='binned'))
    degenerate = np.concatenate([f, np.array([[0, 0, 5], [3, 3, 3]])])      # degenerate triangles never hit
    v1 = vis_case('sphere', 1)[0]
    assert np.array_equal(_vis(lib, device, v1, degenerate, None, mode='binned'), _vis(lib, device, v1, f, None, mode='brute'))


def check_full_size(lib, device):
    """GPU only: the synthetic body model (V = 10475, F = 20908), B = 2 frames in front of the camera"""
    from lemo_amd import synthetic
    import __graft_entry__ as G
    prob = G.prox_small_problem(B=2, V=10475)
    fit = G.prox_fitter_for(prob, device, lib=lib)[0]
    with torch.no_grad():
        body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(2, -1)
        verts = fit.body_model(return_verts=True, body_pose=body_pose).vertices.detach().contiguous()
    faces = synthetic.local_faces(host(verts[0]), 20908).astype(np.int64)      # body-sized mesh: small triangles over the posed vertices
    assert verts.shape == (2, 10475, 3) and faces.shape == (20908, 3) and float(verts[..., 2].min()) > 0.05
    brute = host(vertex_visibility(verts, faces, mode='brute', _lib=lib))
    binned, nbig = vertex_visibility(verts, faces, mode='binned', return_big=True, _lib=lib)
    assert np.array_equal(brute, host(binned))
    sub = np.arange(0, 10475, 10475 // 512)[:512]
    vh = host(verts)
    for b in range(2):
        v64 = vh[b]
        o_s, o_l, o_p = hits64_subset(v64, faces, sub)
        excused = o_s != o_l
        print(f'full size frame {b}: visible {brute[b].mean():.3f}, excused {excused.sum()} of 512, big / thin triangles {int(host(nbig)[b])}')
        assert excused.mean() <= EXCUSE_CAP
        assert not np.any((brute[b, sub].astype(bool) != o_p) & ~excused)


def hits64_subset(v, f, sub):
    """hits64 for the vertices ``sub`` of the frame against all faces"""
    o, test = _rays(v[sub], np.zeros(3), 1e-3, F64)
    v64 = v.astype(F64)
    v0, e1, e2 = v64[f[:, 0]], v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]
    out = [np.ones(len(sub), bool) for _ in range(3)]
    with np.errstate(all='ignore'):
        for lo in range(0, len(sub), 64):
            oo = o[lo:lo + 64]
            D = (-oo)[:, None, :]
            pv = np.cross(D, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo[:, None, :] - v0[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            w = (D * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            for k, m in enumerate((VIS_EPS, -VIS_EPS, 0.0)):
                hit = (det != 0) & (u >= m) & (w >= m) & (u + w <= 1 - m) & (t >= m) & (t <= 1 - m)
                out[k][lo:lo + 64] = ~(hit.any(1) & test[lo:lo + 64])
    return out


# ------------------------------------------------------------------------------------------------------------ masked nearest
MASKED_SHAPES = [(1, 1, 1), (3, 7, 5), (1, _Q + 1, _C + 1), (2, 70, 2 * _L + 7)]


def _valid(B, P, n, m):
    ok = np.ones((B, P), bool)
    if n is not None:
        ok &= np.arange(P)[None, :] < np.asarray(n)[:, None]
    if m is not None:
        ok &= np.asarray(m).astype(bool)
    return ok


def mask_variants(B, N, M):
    """(n1, q_mask, n2, t_mask) sets for one shape: the counts of the issue, single survivors, an empty entry, count and mask together"""
    rng = np.random.default_rng(B * 7 + N + M)
    out = []
    for n2v in sorted({1, min(M, _C - 1), min(M, _C), min(M, _C + 1), M}):
        for n1v in sorted({1, N}):
            out.append((np.full(B, n1v, np.int32), None, np.full(B, n2v, np.int32), None))
    last = np.zeros((B, M), np.uint8)
    last[:, M - 1] = 1
    out.append((None, None, None, last))                          # only the last target survives
    tm = (rng.random((B, M)) < 0.5).astype(np.uint8)
    tm[:, 0] = 1
    qm = (rng.random((B, N)) < 0.6).astype(np.uint8)
    n1, n2 = rng.integers(0, N + 1, B).astype(np.int32), rng.integers(1, M + 1, B).astype(np.int32)
    out.append((n1, qm, n2, tm))                                  # count and mask together: both have to hold
    if B >= 3:
        tm2 = tm.copy()
        tm2[1] = 0                                                # an entry without any valid target
        n1b = np.full(B, N, np.int32)
        n1b[2] = 0                                                # and one without any valid query
        out.append((n1b, None, None, tm2))
    return out


def _points_case(B, N, M, lattice):
    rng = np.random.default_rng(99 + 1000 * B + 10 * N + M + lattice)
    if lattice:
        return rng.integers(-4, 5, (B, N, 3)).astype(F32), rng.integers(-4, 5, (B, M, 3)).astype(F32)
    return (0.8 * rng.standard_normal((B, N, 3)) + 3.0).astype(F32), (1.5 * rng.standard_normal((B, M, 3)) + 3.0).astype(F32)


def _all_pairs(a, b):
    d = a.astype(F64)[:, :, None, :] - b.astype(F64)[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _run_masked(lib, device, a, b, n1, qm, n2, tm, split=0, grad=False):
    t = lambda x, dt=None: None if x is None else dev(x, device, dt)
    A, Bt = dev(a, device).requires_grad_(grad), dev(b, device).requires_grad_(grad)
    d, i = masked_nearest(A, Bt, n1=t(n1), q_mask=t(qm), n2=t(n2), t_mask=t(tm), split=split, _lib=lib)
    return d, i, A, Bt


def check_masked(lib, device, B, N, M, lattice):
    a, b = _points_case(B, N, M, lattice)
    D = _all_pairs(a, b)
    for n1, qm, n2, tm in mask_variants(B, N, M):
        qv, tv = _valid(B, N, n1, qm), _valid(B, M, n2, tm)
        Dm = np.where(tv[:, None, :], D, np.inf)
        live = qv & tv.any(1)[:, None]
        d, i, _, _ = _run_masked(lib, device, a, b, n1, qm, n2, tm)
        d, i = host(d), host(i)
        assert d.dtype == F32 and i.dtype == np.int32 and d.shape == (B, N)
        assert np.all(i[~live] == -1) and np.all(d[~live] == 0.0), 'an invalid query (or an entry without targets) must report 0 / -1'
        assert np.all(i[live] >= 0) and np.all(np.take_along_axis(tv, np.maximum(i, 0).astype(np.int64), 1)[live]), 'an invalid target was chosen'
        at = np.take_along_axis(D, np.maximum(i, 0)[..., None].astype(np.int64), 2)[..., 0]
        mn = Dm.min(2)
        if lattice:
            assert np.array_equal(d[live], mn[live].astype(F32)) and np.array_equal(i[live], Dm.argmin(2)[live]), 'not the lowest valid index'
        else:
            assert np.all(np.abs(d.astype(F64) - at)[live] <= 6 * EPS24 * at[live])
            assert np.all(at[live] <= (1 + 12 * EPS24) * mn[live])
        for split in (1, 2, 3, 7):
            d2, i2, _, _ = _run_masked(lib, device, a, b, n1, qm, n2, tm, split=split)
            assert np.array_equal(host(d2), d) and np.array_equal(host(i2), i), f'split {split} changes the result'
    # everything valid: chamfer_distance, bit for bit
    full = (np.full(B, N, np.int32), np.ones((B, N), np.uint8), np.full(B, M, np.int32), np.ones((B, M), np.uint8))
    want = chamfer_distance(dev(a, device), dev(b, device), bidirectional=False, _lib=lib)
    for args in (full, (None, None, None, None), (full[0], None, None, full[3])):
        d, i, _, _ = _run_masked(lib, device, a, b, *args)
        assert torch.equal(d, want[0]) and torch.equal(i, want[2])


def check_masked_backward(lib, device, B, N, M):
    a, b = _points_case(B, N, M, False)
    rng = np.random.default_rng(5 + N)
    g = rng.standard_normal((B, N)).astype(F32)
    for n1, qm, n2, tm in mask_variants(B, N, M)[-2:]:
        d, i, A, Bt = _run_masked(lib, device, a, b, n1, qm, n2, tm, grad=True)
        (d * dev(g, device)).sum().backward()
        i = host(i)
        a64, b64 = a.astype(F64), b.astype(F64)
        G1, G2, S2, K2 = np.zeros(a.shape), np.zeros(b.shape), np.zeros(b.shape), np.zeros(b.shape[:2])
        for bb in range(B):
            sel = np.nonzero(i[bb] >= 0)[0]
            t = 2.0 * g[bb, sel].astype(F64)[:, None] * (a64[bb, sel] - b64[bb, i[bb, sel]])
            G1[bb, sel] = t
            np.add.at(G2[bb], i[bb, sel], -t); np.add.at(S2[bb], i[bb, sel], np.abs(t)); np.add.at(K2[bb], i[bb, sel], 1)
        g1, g2 = host(A.grad), host(Bt.grad)
        assert np.all(np.abs(g1 - G1) <= 4 * EPS24 * np.abs(G1)), 'own side'
        assert np.all(g1[i < 0] == 0.0), 'an invalid query has a gradient'
        assert np.all(np.abs(g2 - G2) <= 4 * K2[..., None] * EPS24 * S2), 'scatter side'
        assert np.all(g2[K2 == 0] == 0.0), 'a target nobody chose has a gradient'
        if B >= 3 and tm is not None and not tm[1].any():
            assert np.all(g1[1] == 0.0) and np.all(g2[1] == 0.0)


# ------------------------------------------------------------------------------------------------------------ terms
def body_mask_golden():
    ids = np.load(os.path.join(GOLDEN, 'body_mask_ids.npz'))['body_mask_ids']
    assert ids.shape == (5023,) and len(set(ids.tolist())) == 5023 and ids.min() >= 0 and ids.max() < 10475
    return ~np.isin(np.arange(10475), ids)                        # fit_temp_loadprox_slide.py:421-426: the body is the complement


def terms_reference(verts, vis, scan, spn, body_mask, ws, wm, rs, rm):
    """float64 torch restatement of fitting_temp_slide.py:650-670 on the kernel's visibility: per-frame compaction, all pairs, GMoF
    on the squared distance, means; frames without a visible vertex or a scan point are left out"""
    v = torch.from_numpy(verts.astype(F64)).requires_grad_(True)
    s = torch.from_numpy(scan.astype(F64))
    s2m, m2s = [], []
    for b in range(verts.shape[0]):
        vb = torch.from_numpy(vis[b].astype(bool))
        if int(spn[b]) == 0 or int(vb.sum()) == 0:
            continue
        sc = s[b, :int(spn[b])]
        D = ((sc[:, None, :] - v[b][None, vb, :]) ** 2).sum(-1)
        s2m.append(gmof(D.min(1).values, rs).mean())
        sel = vb & torch.from_numpy(body_mask)
        if int(sel.sum()):
            D2 = ((v[b][sel][:, None, :] - sc[None]) ** 2).sum(-1)
            m2s.append(gmof(D2.min(1).values, rm).mean())
    z = torch.zeros((), dtype=torch.float64)
    a = ws * torch.stack(s2m).mean() if s2m and ws > 0 else z
    c = wm * torch.stack(m2s).mean() if m2s and wm > 0 else z
    if (a + c).requires_grad:
        (a + c).backward()
    return float(a.detach()), float(c.detach()), (v.grad.numpy() if v.grad is not None else np.zeros(verts.shape))


def terms_case(coincide=False):
    sv, f = icosphere()
    B, V, S = 3, len(sv), 400
    rng = np.random.default_rng(17)
    verts = np.stack([sv * 0.5 + np.array([0.1 * k, -0.05, 3.0 + 0.1 * k]) for k in range(B)]).astype(F32)
    scan = np.zeros((B, S, 3), F32)
    for b in range(B):
        front = np.nonzero(sv[:, 2] < -0.3)[0]
        pick = rng.choice(front, S)
        scan[b] = verts[b, pick] + rng.normal(0, 0.01, (S, 3)).astype(F32)
    if coincide:
        scan[0, 5] = verts[0, np.nonzero(sv[:, 2] < -0.9)[0][0]]     # d == 0 on a visible vertex
    spn = np.array([S, S // 2, 0], np.int32)
    scan[1, S // 2:] = 0.0
    scan[2] = 0.0                                                 # the padding of fit_temp_loadprox_slide: zeros
    body_mask = np.ones(V, bool)
    body_mask[rng.permutation(V)[:V // 3]] = False
    return verts, f, scan, spn, body_mask


class _Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def check_terms(lib, device, monkeypatch, coincide):
    verts, f, scan, spn, body_mask = terms_case(coincide)
    ws, wm, rs, rm = 1.3, 0.7, 0.2, 0.1
    vis = host(vertex_visibility(dev(verts, device), f, _lib=lib))
    recs = {n: _Recorder(getattr(lib, n)) for n in ('vertex_visibility', 'chamfer_masked_forward')}
    for n, r in recs.items():
        monkeypatch.setattr(lib, n, r)
    args = (f, dev(scan, device), dev(spn, device), dev(body_mask, device))
    for w_s, w_m, nvis, nnn in ((ws, wm, 1, 2), (ws, 0.0, 1, 1), (0.0, wm, 1, 1), (0.0, 0.0, 0, 0)):
        for r in recs.values():
            r.calls = 0
        v = dev(verts, device).requires_grad_(True)
        s2m, m2s = scan_terms(v, args[0], args[1], args[2], args[3], w_s, w_m, rs, rm, _lib=lib)
        assert recs['vertex_visibility'].calls == nvis and recs['chamfer_masked_forward'].calls == nnn, (w_s, w_m)
        a, c, gw = terms_reference(verts, vis, scan, spn, body_mask, w_s, w_m, rs, rm)
        if w_s == 0:
            assert float(s2m) == 0.0
        if w_m == 0:
            assert float(m2s) == 0.0
        if w_s == 0 and w_m == 0:
            continue
        (s2m + m2s).backward()
        g = host(v.grad)
        for got, want, what in ((float(s2m), a, 's2m'), (float(m2s), c, 'm2s')):
            if want:
                print(f'{what} (coincide={coincide}): {got:.8f} vs {want:.8f}, rel {abs(got - want) / want:.2e} (bound 1e-5)')
                assert abs(got - want) <= 1e-5 * want
        ge = float(np.abs(g - gw).max() / np.abs(gw).max())
        print(f'  gradient rel {ge:.2e} (bound 1e-5)')
        assert np.isfinite(g).all() and ge <= 1e-5
        assert np.all(g[2] == 0.0)                                # the frame without scan points drops out
    monkeypatch.undo()
    if coincide:
        d, _ = masked_nearest(dev(scan, device), dev(verts, device), n1=dev(spn, device), t_mask=dev(vis, device), _lib=lib)
        assert float(d[0, 5]) == 0.0
        x = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        gmof(x, 0.2).sum().backward()
        assert torch.isfinite(x.grad).all() and float(x.grad[0]) == 1.0


def check_prox_fitter(lib, device, monkeypatch):
    """ProxTemporalFitter with a scan on the B = 14 golden setup of chamfer_common.check_prox_fitter"""
    import __graft_entry__ as G
    import lemo_amd.prox as P
    prob = G.prox_small_problem(B=14, V=10475)
    real = P.ProxTemporalFitter

    def fitter(**kw):
        monkeypatch.setattr(P, 'ProxTemporalFitter', lambda *a, **k: real(*a, **k, **kw))
        try:
            return G.prox_fitter_for(prob, device, lib=lib)[0]
        finally:
            monkeypatch.setattr(P, 'ProxTemporalFitter', real)

    recs = {n: _Recorder(getattr(lib, n)) for n in ('vertex_visibility', 'chamfer_masked_forward')}
    for n, r in recs.items():
        monkeypatch.setattr(lib, n, r)
    plain = fitter()
    with torch.no_grad():
        base = {k: v.detach().clone() for k, v in plain.loss_dict().items()}
        body_pose = plain.vposer.decode(plain.pose_embedding, output_type='aa').view(14, -1)
        verts = plain.body_model(return_verts=True, body_pose=body_pose).vertices.detach()
    assert float(base['s2m_dist']) == 0.0 and float(base['m2s_dist']) == 0.0
    S = 256
    g = torch.Generator().manual_seed(3)
    pick = torch.randint(0, 10475, (14, S), generator=g).to(device)
    scan = torch.gather(verts, 1, pick[..., None].expand(-1, -1, 3)) + 0.02 * torch.randn(14, S, 3, generator=g).to(device)
    spn = torch.full((14,), S, dtype=torch.int32, device=device)
    spn[3] = S // 2
    mask = dev(body_mask_golden(), device)
    same = lambda ld: set(ld) == set(base) and all(torch.equal(ld[k].detach(), base[k]) for k in base)
    fit = fitter(scan=scan, scan_point_num=spn, body_mask=mask)
    with torch.no_grad():
        assert same(fit.loss_dict())                              # a scan without a weight
    plain.w['s2m_weight'] = 1.0                                   # a weight without a scan
    with torch.no_grad():
        assert same(plain.loss_dict())
    assert all(r.calls == 0 for r in recs.values()), 'a scan kernel ran without scan or weight'
    fit.w.update(s2m_weight=2.0, m2s_weight=3.0, rho_s2m=0.2, rho_m2s=0.1)
    t0 = fit.body_model.transl.detach().clone()
    ld = fit.closure()
    with torch.no_grad():
        s2m, m2s = scan_terms(verts, np.asarray(fit.body_model.faces), scan, spn, mask, 2.0, 3.0, 0.2, 0.1, _lib=lib)
    print(f'PROX window B = 14: s2m {float(s2m):.6f}, m2s {float(m2s):.6f}, total {float(base["total_loss"]):.6f} -> {float(ld["total_loss"]):.6f}')
    assert float(s2m) > 0 and float(m2s) > 0
    assert torch.equal(ld['s2m_dist'].detach() + ld['m2s_dist'].detach(), s2m + m2s)
    assert torch.equal(ld['total_loss'].detach(), base['total_loss'] + (s2m + m2s)), 'total_loss does not rise by exactly the two terms'
    for k in base:
        if k not in ('total_loss', 's2m_dist', 'm2s_dist'):
            assert torch.equal(ld[k].detach(), base[k]), k
    fit.optimizer.step()
    assert torch.isfinite(fit.body_model.transl).all() and not torch.equal(fit.body_model.transl.detach(), t0)
    monkeypatch.undo()


def check_compat(lib, device, monkeypatch):
    import lemo_amd.compat as compat
    import lemo_amd.compat.psbody.mesh.visibility as pv
    monkeypatch.setattr(pv, '_lib', lib)
    saved = {k: sys.modules.get(k) for k in ('psbody', 'psbody.mesh', 'psbody.mesh.visibility')}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        compat.install()
        from psbody.mesh import Mesh
        from psbody.mesh.visibility import visibility_compute
        verts, f, _ = vis_case('two_spheres', 1)
        m = Mesh(v=verts[0], f=f)
        vis, n_dot = visibility_compute(v=m.v, f=m.f, cams=np.zeros((1, 3)))          # fitting_temp_slide.py:648-649
        assert vis.dtype == np.uint32 and vis.shape == (1, verts.shape[1]) and n_dot.shape == vis.shape and not n_dot.any()
        assert np.array_equal(vis.squeeze().astype(np.uint8), _vis(lib, device, verts, f, None)[0])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        monkeypatch.undo()


def check_validation(lib, device, monkeypatch):
    launched = []
    for name in ('vertex_visibility', 'chamfer_masked_forward', 'chamfer_backward'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    verts, f, scan, spn, body_mask = terms_case()
    B, V, S = verts.shape[0], verts.shape[1], scan.shape[1]
    v, s, n, m = dev(verts, device), dev(scan, device), dev(spn, device), dev(body_mask, device)
    E = (ValueError, _hip.LemoHipError)
    for kw in (dict(vertices=v.double()), dict(vertices=v[0]), dict(vertices=host(v)), dict(faces=f.astype(F64)), dict(faces=f[:, :2]),
               dict(faces=np.concatenate([f, [[0, 1, V]]])), dict(faces=np.concatenate([f, [[0, -1, 2]]])), dict(mode='fast'), dict(grid=1),
               dict(grid=65), dict(min_dist=-1.0), dict(min_dist=float('nan')), dict(cam=np.zeros(2)), dict(faces=dev(f, device, np.int64))):
        args = dict(vertices=v, faces=f, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            vertex_visibility(**args)
    for kw in (dict(xyz1=s.double()), dict(xyz2=v[:2]), dict(n1=spn), dict(n1=n.long()), dict(n1=n[:2]), dict(q_mask=m), dict(t_mask=m.float()[None]),
               dict(t_mask=torch.ones(B, V + 1, dtype=torch.uint8, device=device)), dict(split=-1), dict(xyz1=None)):
        args = dict(xyz1=s, xyz2=v, n1=n, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            masked_nearest(**args)
    for kw in (dict(scan=s.double()), dict(scan=s[:2]), dict(scan_point_num=dev(spn + S, device)), dict(scan_point_num=n.long()),
               dict(scan_point_num=spn), dict(body_mask=m[:-1]), dict(body_mask=m.to(torch.uint8)), dict(vertices=v.half()),
               dict(faces=np.concatenate([f, [[0, 1, V]]])), dict(s2m_weight=-1.0), dict(scan_point_num=dev(spn - 1, device))):
        args = dict(vertices=v, faces=f, scan=s, scan_point_num=n, body_mask=m, s2m_weight=1.0, m2s_weight=1.0, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            scan_terms(**args)
    if device.type != 'cpu':
        with pytest.raises(E):
            vertex_visibility(v.cpu(), f, _lib=lib)
        with pytest.raises(E):
            scan_terms(v, f, s.cpu(), n, m, 1.0, 1.0, _lib=lib)
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    vv = lambda B=1, V=1, F=1, mode=0, grid=0, x=1, md=1e-3, ws=None, wsb=0: lib.vertex_visibility(x, B, V, 1, F, None, md, mode, grid, 1, None, ws, wsb, None)
    assert vv(B=0) == 10001 and vv(V=0) == 10001 and vv(F=0) == 10001 and vv(B=65536) == 10001
    assert vv(mode=3) == 10002 and vv(grid=1) == 10002 and vv(grid=65) == 10002 and vv(x=None) == 10002 and vv(md=-1.0) == 10002
    assert vv(mode=2) == 10002                                     # binned without its workspace
    assert lib.vertex_visibility_workspace_bytes(1, 0, 1, 0, 0) == -1 and lib.vertex_visibility_workspace_bytes(1, 1, 1, 1, 0) == 0
    assert lib.vertex_visibility_workspace_bytes(2, 10, 5, 2, 4) == 2 * 4 * (8 + 16 + 1 + 40)
    mf = lambda B=1, N=1, M=1, split=0, x=1: lib.chamfer_masked_forward(x, 1, B, N, M, None, None, None, None, split, 1, 1, None, 0, None)
    assert mf(N=0) == 10001 and mf(B=65536) == 10001 and mf(x=None) == 10002 and mf(split=-1) == 10002 and mf(M=4096, split=2) == 10002
