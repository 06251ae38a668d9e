"""Cases and yardsticks for lemo_amd.selfpen (csrc/selfpen_kernels.hip), shared by tests/test_selfpen_emu.py (host emulator) and
tests/test_selfpen_gpu.py (MI355X).  mesh_intersection (torch-mesh-isect) is neither under the reference tree nor installed: the
yardsticks are float64 restatements of the definitions the kernel file states, written for these tests.

Search.  ``collide64``: all pairs i < j without a shared vertex index, six segment / triangle tests by the textbook Moeller-Trumbore
in float64 (u, v, t by division), evaluated strict (u, v >= eps, u + v <= 1 - eps, eps <= t <= 1 - eps), loose (the same with -eps)
and plain.  A pair is EXCUSED iff strict != loose; everywhere else the kernel's set must equal the plain float64 set.  eps by
scan_common's method: ``measure_eps`` looks for the smallest power of two for which ``collide32`` -- the kernel's own formulation
(no division, boxes first) in unfused float32 numpy -- disagrees with float64 only on excused pairs, over all mesh cases below.
Measured: NO disagreement at all on these cases, down to the floor of the search, 2^-30.  A measurement that finds nothing cannot set
the margin, so it comes from the number format: the corners are fp32, differences of nearby corners are exact or carry 2^-24 of
their own size, so each of det, u det, v det, t det (a triple product of three such differences) carries about 8 roundings, 2^-21 of
|d| |e1| |e2|; det itself is |d| |e1| |e2| times the sine of the triangle's corner and the cosine of the segment's angle to the
normal, above 2^-4 for meshes without slivers away from grazing incidence: 2^-17 on u, v, t.  SP_EPS = 4 x that = 2^-15, the margin
scan_common gives the visibility suite.  Excused pairs are capped at 1 % of each case's float64 colliding pairs and every mesh case has
at least 100 of those; both are conditions on the poses that the float64 yardstick alone meets (asserted).

Loss.  ``loss64``: the definition in float64 torch with autograd, in camera coordinates, handed the kernel's own pair list.  L within
1e-5 relative (the project's loss-scalar tolerance).  Gradient: max |g - g64| / max |g64| over the frame; the bound is
4 x what the SAME restatement evaluated in float32 (``loss64(..., dtype=torch.float32)``) shows against float64 on these cases.
Measured with ``measure_grad_bound()``: see GRAD32_MEASURED below.
"""
import functools
import sys

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd import selfpen as SP
from lemo_amd.selfpen import find_collisions, ign_table, penetration_loss, segmentation_from_weights, self_penetration_term
from scan_common import _Recorder, dev, host, icosphere, rot, torus

F32, F64 = np.float32, np.float64
SP_EPS_DERIVED = 2.0 ** -17
SP_EPS = 4 * SP_EPS_DERIVED
EXCUSE_CAP = 0.01
MIN_PAIRS = 100
LOSS_TOL = 1e-5
GRAD32_MEASURED = 5.3e-4          # measure_grad_bound() -> (loss 1.2e-6, gradient 5.23e-4): the float32 restatement forms the circumcentre in
                                  # camera coordinates, 3 m from the origin, and sigma = 1e-4 multiplies what that loses by r / sigma
GRAD_TOL = 4 * GRAD32_MEASURED
SIGMAS = (1e-4, 0.5)


# ------------------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def sp_case(name, B):
    """-> (verts float32 [B, V, 3], faces int64 [F, 3]); the frames are rigid moves of one another with generic offsets"""
    if name in ('spheres', 'spheres3'):
        sv, sf = icosphere(2 if name == 'spheres' else 3)
        v = np.concatenate([sv * 0.5 + np.array([0.113, -0.047, 3.021]),
                            (sv * np.array([0.75, 0.45, 0.2])) @ rot([0.3, 1.0, 0.2], 0.37).T + np.array([0.331, 0.109, 3.067])])
        # (the second sphere is flattened: a round pair of level-2 spheres cuts in a circle that crosses only ~75 pairs of triangles)
        f = np.concatenate([sf, sf + len(sv)])
    elif name == 'torus_sphere':
        tv, tf = torus()
        sv, sf = icosphere(2)
        v = np.concatenate([tv @ rot([1.0, 0.3, 0.1], 1.05).T + np.array([-0.103, 0.097, 2.513]),
                            (sv @ rot([0.1, 0.2, 1.0], 0.81).T) * 0.31 + np.array([0.281, 0.263, 2.431])])
        f = np.concatenate([tf, sf + len(tv)])
    else:
        raise KeyError(name)
    frames = [v]
    for k in range(1, B):
        frames.append(v @ rot([0.05 * k, 0.02, 1.0], 0.4 * k).T + np.array([0.07 * k, -0.04 * k, 0.15 * k]))
    verts = np.stack(frames).astype(F32)
    verts.setflags(write=False)
    return verts, f


MESH_CASES = [('spheres', 1), ('spheres', 3), ('torus_sphere', 1), ('spheres3', 1)]
LOSS_CASES = [('spheres', 3), ('torus_sphere', 1)]

TRI_A = np.array([[0.0, 0.0, 3.0], [1.0, 0.0, 3.0], [0.0, 1.0, 3.0]])                # centroid (1/3, 1/3, 3)


def tri_pair(lift=0.0, share=False, coplanar=False):
    """two triangles; one edge of the second passes through the centroid of the first (lift = 0), or clear of it"""
    if coplanar:
        b = np.array([[0.2, 0.2, 3.0], [1.2, 0.3, 3.0], [0.3, 1.2, 3.0]])
    else:
        b = np.array([[1 / 3, 1 / 3, 2.5 + lift], [1 / 3, 1 / 3, 3.5 + lift], [1.5, 1 / 3, 3.0 + lift]])
    v = np.concatenate([TRI_A, b])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    if share:
        v = np.concatenate([TRI_A, [[0.25, 0.25, 2.5], [0.25, 0.25, 3.5]]])
        f = np.array([[0, 1, 2], [0, 3, 4]])                      # shares vertex 0, and its far edge crosses the first triangle
    return v[None].astype(F32), f


# ------------------------------------------------------------------------------------------------------------ search yardsticks
def _boxes(p, dt):
    t = p.astype(dt)
    return t.min(1), t.max(1)


def _candidates(v, f, pad):
    """pairs i < j without a shared index whose boxes, inflated by pad, overlap -> (i [n], j [n])"""
    lo, hi = _boxes(v[f], F64)
    ov = np.ones((len(f), len(f)), bool)
    for a in range(3):
        ov &= (lo[:, None, a] - pad <= hi[None, :, a]) & (lo[None, :, a] - pad <= hi[:, None, a])
    share = (f[:, None, :, None] == f[None, :, None, :]).any((2, 3))
    ov &= ~share & np.triu(np.ones_like(ov), 1)
    return np.nonzero(ov)


def _seg_tri64(a, b, v0, v1, v2, margins):
    d, e1, e2 = b - a, v1 - v0, v2 - v0
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    tv = a - v0
    with np.errstate(all='ignore'):
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        w = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
        return [(det != 0) & (u >= m) & (w >= m) & (u + w <= 1 - m) & (t >= m) & (t <= 1 - m) for m in margins]


def collide64(v, f, eps=SP_EPS, segm=None):
    """one frame -> three sets of (i, j): strict, loose, plain"""
    i, j = _candidates(v, f, 1e-3)
    A, Bt = v.astype(F64)[f[i]], v.astype(F64)[f[j]]
    hit = [np.zeros(len(i), bool) for _ in range(3)]
    for P, Q in ((A, Bt), (Bt, A)):
        for k in range(3):
            for n, h in enumerate(_seg_tri64(P[:, k], P[:, (k + 1) % 3], Q[:, 0], Q[:, 1], Q[:, 2], (eps, -eps, 0.0))):
                hit[n] |= h
    keep = np.ones(len(i), bool) if segm is None else ~filtered_numpy(i, j, *segm)
    return [set(zip(i[h & keep].tolist(), j[h & keep].tolist())) for h in hit]


def collide32(v, f):
    """the kernel's own formulation in unfused float32 numpy: exact boxes first, Moeller-Trumbore without a division -> set of (i, j)"""
    i, j = _candidates(v, f, 0.0)
    v = v.astype(F32)
    A, Bt = v[f[i]], v[f[j]]
    hit = np.zeros(len(i), bool)
    with np.errstate(all='ignore'):
        for P, Q in ((A, Bt), (Bt, A)):
            e1, e2 = Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0]
            for k in range(3):
                a, b = P[:, k], P[:, (k + 1) % 3]
                d, tv = b - a, a - Q[:, 0]
                pv, qv = np.cross(d, e2).astype(F32), np.cross(tv, e1).astype(F32)
                det, U, W, T = (e1 * pv).sum(-1, dtype=F32), (tv * pv).sum(-1, dtype=F32), (d * qv).sum(-1, dtype=F32), (e2 * qv).sum(-1, dtype=F32)
                S = U + W
                hit |= ((det > 0) & (U >= 0) & (W >= 0) & (S <= det) & (T >= 0) & (T <= det)) | \
                       ((det < 0) & (U <= 0) & (W <= 0) & (S >= det) & (T <= 0) & (T >= det))
    return set(zip(i[hit].tolist(), j[hit].tolist()))


@functools.lru_cache(maxsize=None)
def reference(name, B):
    verts, f = sp_case(name, B)
    return [collide64(verts[b], f) for b in range(B)]


def measure_eps():
    """the docstring's measurement: smallest power of two for which collide32 disagrees with float64 only on excused pairs"""
    for e in range(30, 5, -1):
        eps, ok = 2.0 ** -e, True
        for name, B in MESH_CASES:
            verts, f = sp_case(name, B)
            for b in range(B):
                s, l, p = collide64(verts[b], f, eps)
                ok = ok and not ((collide32(verts[b], f) ^ p) - (s ^ l))
        if ok:
            return eps
    return None


def filtered_numpy(i, j, segm, parents, ign):
    """the five rules of FilterFaces -> True where the pair is dropped"""
    si, sj = segm[i], segm[j]
    return (si == sj) | (parents[i] == sj) | (parents[j] == si) | (ign[si, sj] != 0) | (ign[sj, si] != 0)


def pair_sets(pairs, count):
    """kernel output -> list of per-frame lists of (i, j), after checking the layout: sorted, -1 behind, count consistent"""
    pairs, count = host(pairs), host(count)
    out = []
    for b in range(pairs.shape[0]):
        n = min(int(count[b]), pairs.shape[1])
        assert np.all(pairs[b, n:] == -1), 'entries behind the last pair must be -1'
        lst = [tuple(r) for r in pairs[b, :n].tolist()]
        assert all(0 <= i < j for i, j in lst) and lst == sorted(set(lst)), 'pairs must be i < j in lexicographic order without repeats'
        out.append(lst)
    return out


def _find(lib, device, verts, f, **kw):
    return find_collisions(dev(verts, device), f, return_count=True, _lib=lib, **kw)


def check_modes_identical(lib, device, verts, f, **kw):
    """brute, grid (two sizes), auto, and faces given as a device tensor: the same bits"""
    base = _find(lib, device, verts, f, mode='brute', **kw)
    for extra in (dict(mode='grid'), dict(mode='grid', grid=5), dict(mode='grid', grid=2), dict(mode='auto')):
        got = _find(lib, device, verts, f, **extra, **kw)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), f'{extra} differs from brute force'
    ft = f if isinstance(f, torch.Tensor) else dev(f, device, np.int32)
    got = find_collisions(dev(verts, device), ft, return_count=True, mode='grid', grid=7, _lib=lib, **kw)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    return base


def check_search(lib, device, name, B):
    verts, f = sp_case(name, B)
    pairs, count = check_modes_identical(lib, device, verts, f, max_pairs=4096)
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (B, 4096, 2) and count.dtype == torch.int32
    got = pair_sets(pairs, count)
    for b, (strict, loose, plain) in enumerate(reference(name, B)):
        excused = strict ^ loose
        print(f'{name} B = {B} frame {b}: {len(plain)} float64 pairs, kernel {len(got[b])}, excused {len(excused)}')
        assert len(plain) >= MIN_PAIRS, f'{name}: only {len(plain)} colliding pairs'
        assert len(excused) <= EXCUSE_CAP * len(plain), f'{name}: {len(excused)} excused pairs of {len(plain)}'
        assert int(host(count)[b]) == len(got[b])
        bad = (set(got[b]) ^ plain) - excused
        assert not bad, f'{name}: {len(bad)} pairs differ from float64 outside the excuse set, e.g. {sorted(bad)[:4]}'


def check_capacity(lib, device):
    verts, f = sp_case('spheres', 3)
    full, count = _find(lib, device, verts, f, max_pairs=4096)
    n = host(count)
    C = int(n.min()) // 2 + 1
    assert C < n.min()
    for mode in ('brute', 'grid'):
        part, cnt = _find(lib, device, verts, f, max_pairs=C, mode=mode)
        assert torch.equal(cnt, count), 'count must stay the true number'
        assert torch.equal(part, full[:, :C]), 'not the first C pairs in order'
    one, cnt = _find(lib, device, verts, f, max_pairs=1)
    assert torch.equal(one, full[:, :1]) and torch.equal(cnt, count)


def check_closed_form(lib, device):
    for kw, want in ((dict(), [(0, 1)]), (dict(lift=0.75), []), (dict(share=True), []), (dict(coplanar=True), [])):
        v, f = tri_pair(**kw)
        pairs, count = check_modes_identical(lib, device, v, f, max_pairs=4)
        assert pair_sets(pairs, count)[0] == want, (kw, host(pairs))
        assert collide64(v[0], f)[2] == set(want), kw
    v, f = tri_pair(share=True)
    f2 = np.array([[0, 1, 2], [5, 3, 4]])                         # the same geometry without the shared index: the far edge does cross
    v2 = np.concatenate([v[0], v[0][:1]])[None]
    assert pair_sets(*_find(lib, device, v2, f2, max_pairs=4))[0] == [(0, 1)]
    # a face that names a missing vertex, a degenerate face and a NaN corner never collide (device faces are not checked on the host)
    v, f = tri_pair()
    fd = dev(np.array([[0, 1, 2], [3, 4, 5], [3, 4, 99], [3, 3, 5], [3, 4, -1]]), device, np.int32)
    assert pair_sets(*check_modes_identical(lib, device, v, fd, max_pairs=4))[0] == [(0, 1)]
    vn = v.copy()
    vn[0, 5, 1] = np.nan
    assert pair_sets(*check_modes_identical(lib, device, vn, f, max_pairs=4))[0] == []


def three_part_segmentation():
    """the sphere pair in three parts: sphere 0 below / above its equator (parts 0, 1), sphere 1 (part 2); parents 0 <- 1, 2 free"""
    verts, f = sp_case('spheres', 1)
    nf = len(f) // 2
    cz = verts[0][f].mean(1)[:, 1]
    segm = np.where(np.arange(len(f)) >= nf, 2, (cz[:] > cz[:nf].mean()).astype(int)).astype(np.int32)
    parents = np.array([-1, 0, -1], np.int32)[segm]
    return segm, parents


def check_filter(lib, device):
    verts, f = sp_case('spheres', 1)
    segm, parents = three_part_segmentation()
    plain = pair_sets(*_find(lib, device, verts, f, max_pairs=4096))[0]
    assert len(plain) >= MIN_PAIRS
    i, j = np.array(plain).T
    seen = set()
    for ign_list in (None, ['0,2'], ['2,1'], ['0,2', '1,2']):
        ign = ign_table(ign_list, 3)
        want = [p for p, d in zip(plain, filtered_numpy(i, j, segm, parents, ign)) if not d]
        kw = dict(faces_segm=segm, faces_parents=parents, ign_part_pairs=ign_list)
        got = pair_sets(*check_modes_identical(lib, device, verts, f, max_pairs=4096, **kw))[0]
        assert got == want, ign_list
        seen.add(len(got))
    assert 0 in seen and len(seen) >= 3, seen                      # one table removes every pair; the others remove different shares
    same = np.zeros(len(f), np.int32)                              # one part: everything goes
    assert pair_sets(*_find(lib, device, verts, f, max_pairs=64, faces_segm=same))[0] == []
    # a part and its parent: make sphere 1 the child of part 1
    par2 = np.array([-1, 0, 1], np.int32)[segm]
    want = [p for p, d in zip(plain, filtered_numpy(i, j, segm, par2, ign_table(None, 3))) if not d]
    assert pair_sets(*_find(lib, device, verts, f, max_pairs=4096, faces_segm=segm, faces_parents=dev(par2, device)))[0] == want
    assert 0 < len(want) < len(plain)
    assert np.array_equal(ign_table(['9,16', '9,17'])[9, 15:18], [0, 1, 1]) and ign_table(['9,16']).shape == (64, 64)
    w = np.zeros((4, 3)); w[[0, 1, 2, 3], [2, 0, 1, 1]] = 1
    s, p = segmentation_from_weights(w, np.array([[0, 1, 2], [3, 0, 1]]), np.array([-1, 0, 1]))
    assert s.tolist() == [2, 1] and p.tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------------------ loss yardstick
def loss64(verts, faces, pairs, sigma, outside, dtype=torch.float64, weights=None):
    """the definition in torch with autograd -> (L [B] numpy float64, gradient [B, V, 3] of sum(weights * L))"""
    v = torch.from_numpy(np.asarray(verts)).to(dtype).requires_grad_(True)
    f = torch.from_numpy(np.asarray(faces, np.int64))
    out = []
    for b in range(v.shape[0]):
        pr = torch.tensor(pairs[b], dtype=torch.long).reshape(-1, 2)
        tri = v[b][f]                                             # [F, 3, 3]
        tot = torch.zeros((), dtype=dtype)
        for r, p in ((0, 1), (1, 0)):
            R, P = tri[pr[:, r]], tri[pr[:, p]]
            area = torch.linalg.cross(R[:, 1] - R[:, 0], R[:, 2] - R[:, 0]).detach().norm(dim=-1) > 0
            R, P = R[area], P[area]                                # a zero-area triangle contributes nothing
            p0, p1, p2 = R[:, 0], R[:, 1], R[:, 2]
            N = torch.linalg.cross(p1 - p0, p2 - p0)
            A2 = N.norm(dim=-1)
            ok = A2 > 0
            A2s = torch.where(ok, A2, torch.ones_like(A2))
            n = N / A2s[:, None]
            a2, b2, c2 = ((p1 - p2) ** 2).sum(-1), ((p2 - p0) ** 2).sum(-1), ((p0 - p1) ** 2).sum(-1)
            w0, w1, w2 = a2 * (b2 + c2 - a2), b2 * (c2 + a2 - b2), c2 * (a2 + b2 - c2)
            ws = torch.where(ok, w0 + w1 + w2, torch.ones_like(w0))
            o = (w0[:, None] * p0 + w1[:, None] * p1 + w2[:, None] * p2) / ws[:, None]
            rad = torch.sqrt(a2 * b2 * c2 + (~ok).to(dtype)) / (2 * A2s)
            d = P - o[:, None, :]                                  # [n, 3 corners, 3]
            h = (d * n[:, None, :]).sum(-1)
            q = d - h[..., None] * n[:, None, :]
            rho = torch.sqrt((q * q).sum(-1) + 1e-300 * (dtype == torch.float64))
            D = rad[:, None] - (rad[:, None] / sigma) * h
            Ds = torch.where(D > 0, D, torch.ones_like(D))
            phi = rho / Ds
            k2, k1 = (1 - 2 * sigma) / (4 * sigma * sigma), 1 / (2 * sigma)
            ups = torch.where(h <= -sigma, -h + 1 - sigma, torch.where(h < sigma, -k2 * h * h - k1 * h + (3 - 2 * sigma) / 4, torch.zeros_like(h)))
            if not outside:
                ups = torch.where(h > 0, torch.zeros_like(ups), ups)
            psi = torch.where((D > 0) & (phi < 1) & ok[:, None], (1 - phi) * ups, torch.zeros_like(ups))
            tot = tot + (psi ** 2).sum()
        out.append(tot)
    L = torch.stack(out)
    wts = torch.ones(len(out), dtype=dtype) if weights is None else torch.as_tensor(weights).to(dtype)
    if L.requires_grad:
        (L * wts).sum().backward()
    g = v.grad.double().numpy() if v.grad is not None else np.zeros(np.asarray(verts).shape)
    return L.detach().double().numpy(), g


@functools.lru_cache(maxsize=None)
def _ref_pairs(name, B):
    return [sorted(r[2]) for r in reference(name, B)]


def measure_grad_bound():
    """float32 restatement against float64 on LOSS_CASES: -> (largest relative loss error, largest relative gradient error)"""
    el, eg = 0.0, 0.0
    for name, B in LOSS_CASES:
        verts, f = sp_case(name, B)
        pairs = _ref_pairs(name, B)
        for sigma in SIGMAS:
            for outside in (True, False):
                L64, g64 = loss64(verts, f, pairs, sigma, outside)
                L32, g32 = loss64(verts, f, pairs, sigma, outside, torch.float32)
                el = max(el, float(np.max(np.abs(L32 - L64) / np.maximum(L64, 1e-300))))
                for b in range(B):
                    if np.abs(g64[b]).max() > 0:
                        eg = max(eg, float(np.abs(g32[b] - g64[b]).max() / np.abs(g64[b]).max()))
    return el, eg


def check_loss(lib, device, name, B, sigma, outside):
    verts, f = sp_case(name, B)
    pairs, count = _find(lib, device, verts, f, max_pairs=4096)
    lists = pair_sets(pairs, count)
    wts = np.linspace(0.7, 1.9, B)
    v = dev(verts, device).requires_grad_(True)
    L = penetration_loss(v, f, pairs, count, sigma, outside, _lib=lib)
    assert L.dtype == torch.float32 and tuple(L.shape) == (B,)
    (L * dev(wts, device, F32)).sum().backward()
    L64, g64 = loss64(verts, f, lists, sigma, outside, weights=wts)
    g = host(v.grad).astype(F64)
    for b in range(B):
        rel = abs(float(L[b]) - L64[b]) / L64[b]
        ge = float(np.abs(g[b] - g64[b]).max() / np.abs(g64[b]).max())
        print(f'{name} sigma {sigma} outside {outside} frame {b}: L {float(L[b]):.8g} vs {L64[b]:.8g}, rel {rel:.2e} (bound {LOSS_TOL}); gradient rel {ge:.2e} (bound {GRAD_TOL:.1e})')
        assert L64[b] > 0 and rel <= LOSS_TOL
        assert np.isfinite(g[b]).all() and ge <= GRAD_TOL
    # the list without its count (every entry, -1 skipped) gives the same bits
    L2 = penetration_loss(dev(verts, device), f, pairs, None, sigma, outside, _lib=lib)
    assert torch.equal(L2, L.detach())


def check_loss_edges(lib, device):
    sigma = 0.5
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])            # normal +z, circumcentre (0.5, 0.5, 0), r = sqrt(0.5)
    at = lambda p: np.array([p, p, p], F64)                       # a zero-area second triangle: its own cone contributes nothing, and its
                                                                  # three equal corners are weighed by the first triangle's cone

    def L_of(points, outside=True, s=sigma, grad=False):
        v = dev(np.concatenate([tri, points])[None].astype(F32), device).requires_grad_(grad)
        pr = dev(np.array([[[0, 1]]]), device, np.int32)
        L = penetration_loss(v, np.array([[0, 1, 2], [3, 4, 5]]), pr, None, s, outside, _lib=lib)
        return L, v

    # h = +sigma exactly (the denominator is 0, Upsilon is 0) and a point with Phi >= 1 contribute 0.  h = -sigma is the junction of the two
    # branches of Upsilon, where both give 1, and the denominator is 2 r there: on the axis Psi = 1 - 0, so three corners give exactly 3
    # (the definition leaves no way for that point to give 0; the float64 restatement agrees)
    for p, want in (([50.0, 50.0, 9.0], 0.0), ([0.5, 0.5, sigma], 0.0), ([0.5 + 3.0, 0.5, -0.25], 0.0), ([0.5, 0.5, -sigma], 3.0)):
        got = float(L_of(at(p))[0])
        ref = loss64(np.concatenate([tri, at(p)])[None], np.array([[0, 1, 2], [3, 4, 5]]), [[(0, 1)]], sigma, True)[0][0]
        assert got == want and abs(ref - want) <= 1e-12, (p, got, ref, want)
    assert float(L_of(at([0.5, 0.5, 0.25]), True)[0]) > 0 and float(L_of(at([0.5, 0.5, 0.25]), False)[0]) == 0.0     # h > 0: outside
    assert float(L_of(at([0.5, 0.5, -0.25]), False)[0]) > 0
    # empty lists: exact zero, zero gradient, finite
    verts, f = sp_case('spheres', 3)
    v = dev(verts, device).requires_grad_(True)
    empty = torch.full((3, 8, 2), -1, dtype=torch.int32, device=device)
    for cnt in (torch.zeros(3, dtype=torch.int32, device=device), None):
        L = penetration_loss(v, f, empty, cnt, 1e-4, _lib=lib)
        assert torch.all(L == 0)
        v.grad = None
        L.sum().backward()
        assert torch.all(v.grad == 0) and torch.isfinite(v.grad).all()
    # a degenerate triangle in a pair: finite, and the degenerate triangle's cone contributes nothing and gets no gradient
    deg = np.array([[0.5, 0.5, -0.25], [0.5, 0.5, -0.25], [0.7, 0.2, -0.1]])
    L, v = L_of(deg, grad=True)
    L.sum().backward()
    assert torch.isfinite(L).all() and torch.isfinite(v.grad).all() and float(L) > 0
    ref, gref = loss64(np.concatenate([tri, deg])[None], np.array([[0, 1, 2], [3, 4, 5]]), [[(0, 1)]], sigma, True)
    assert abs(float(L) - ref[0]) <= LOSS_TOL * ref[0] and np.abs(host(v.grad) - gref).max() <= GRAD_TOL * np.abs(gref).max()
    assert torch.all(v.grad[0, 3] == v.grad[0, 4])              # the twin corners: the same point gradient, nothing through their own cone
    both = np.concatenate([[[0.0, 0.0, 0.0]] * 3, deg])[None].astype(F32)     # both triangles without area
    v = dev(both, device).requires_grad_(True)
    L = penetration_loss(v, np.array([[0, 1, 2], [3, 4, 5]]), dev(np.array([[[0, 1]]]), device, np.int32), None, sigma, _lib=lib)
    L.sum().backward()
    assert float(L) == 0.0 and torch.all(v.grad == 0)
    with pytest.raises(NotImplementedError):
        penetration_loss(v, np.array([[0, 1, 2], [3, 4, 5]]), dev(np.array([[[0, 1]]]), device, np.int32), None, sigma, point2plane=True, _lib=lib)
    with pytest.raises(NotImplementedError):
        penetration_loss(v, np.array([[0, 1, 2], [3, 4, 5]]), dev(np.array([[[0, 1]]]), device, np.int32), None, sigma, linear_max=1.0, _lib=lib)


def check_term(lib, device):
    verts, f = sp_case('spheres', 3)
    v = dev(verts, device).requires_grad_(True)
    t = self_penetration_term(v, f, 0.3, sigma=0.5, _lib=lib)
    pairs, count = _find(lib, device, verts, f, max_pairs=SP.DEFAULT_MAX_PAIRS)
    L = penetration_loss(dev(verts, device), f, pairs, count, 0.5, _lib=lib)
    assert torch.equal(t.detach(), torch.sum(0.3 * L)) and float(t) > 0
    t.backward()
    assert torch.isfinite(v.grad).all() and float(v.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ fitter
SP_ENTRIES = ('selfpen_search', 'selfpen_loss_forward', 'selfpen_loss_backward')


def _fitter_setup(lib, device, monkeypatch):
    import __graft_entry__ as G
    import lemo_amd.prox as P
    from lemo_amd import synthetic
    prob = G.prox_small_problem(B=14, V=10475)
    real = P.ProxTemporalFitter

    def fitter(**kw):
        monkeypatch.setattr(P, 'ProxTemporalFitter', lambda *a, **k: real(*a, **k, **kw))
        try:
            return G.prox_fitter_for(prob, device, lib=lib)[0]
        finally:
            monkeypatch.setattr(P, 'ProxTemporalFitter', real)

    def posed(fit):
        with torch.no_grad():
            body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(14, -1)
            return fit.body_model(return_verts=True, body_pose=body_pose).vertices.detach().contiguous()

    # the model's own faces are random index triples (body-sized triangles that all overlap); a surface-sized mesh over the posed cloud
    faces = synthetic.local_faces(host(posed(fitter()))[0], 1200)
    prob['model'] = dict(prob['model'], f=faces)
    return prob, fitter, posed, faces


def smooth_reference(markers, w_vel, w_acc):
    m = markers.astype(F64)
    vel = m[1:] - m[:-1]
    acc = vel[1:] - vel[:-1]
    return float((vel ** 2).mean() * w_vel), float((acc ** 2).mean() * w_acc)


def check_prox_fitter(lib, device, monkeypatch):
    prob, fitter, posed, faces = _fitter_setup(lib, device, monkeypatch)
    recs = {n: _Recorder(getattr(lib, n)) for n in SP_ENTRIES}
    for n, r in recs.items():
        monkeypatch.setattr(lib, n, r)
    plain = fitter()
    with torch.no_grad():
        base = {k: v.detach().clone() for k, v in plain.loss_dict().items()}
    for k in ('self_penetration_loss', 'smooth_vel_loss', 'smooth_acc_loss'):
        assert float(base[k]) == 0.0
    same = lambda ld: set(ld) == set(base) and all(torch.equal(ld[k].detach(), base[k]) for k in base)
    segm, parents = segmentation_from_weights(prob['model']['weights'], faces, np.where(SYN_PARENTS() < 0, -1, SYN_PARENTS()))
    cfg = dict(sigma=0.5, penalize_outside=True, max_pairs=2048)
    seg = dict(faces_segm=segm, faces_parents=parents, ign_part_pairs=['9,16'])
    fit = fitter(selfpen=cfg, **seg)
    with torch.no_grad():
        assert same(fit.loss_dict())                              # configured, but no weight
        fit.w['coll_loss_weight'] = 0.0
        assert same(fit.loss_dict())
    assert all(r.calls == 0 for r in recs.values()), 'a selfpen kernel ran without a weight'
    verts = posed(fit)
    pairs, count = find_collisions(verts, faces, max_pairs=2048, return_count=True, _lib=lib, **seg)
    assert int(count[2:].min()) >= 1, 'the pose has no colliding pair'      # (frame 0, whose cloud the faces were built over, has none)
    fit.w['coll_loss_weight'] = 0.01
    t0 = fit.body_model.transl.detach().clone()
    before = {n: r.calls for n, r in recs.items()}
    ld = fit.closure()
    assert all(recs[n].calls == before[n] + 1 for n in SP_ENTRIES), 'one search, one loss forward and one backward per closure'
    with torch.no_grad():
        want = torch.sum(0.01 * penetration_loss(verts, faces, pairs, count, 0.5, True, _lib=lib))
    print(f'PROX window B = 14: pairs per frame {host(count).tolist()}, self_penetration_loss {float(want):.6g}, total {float(base["total_loss"]):.6f} -> {float(ld["total_loss"]):.6f}')
    assert float(want) > 0 and torch.equal(ld['self_penetration_loss'].detach(), want)
    assert torch.equal(ld['total_loss'].detach(), base['total_loss'] + want), 'total_loss does not rise by exactly the term'
    for k in base:
        if k not in ('total_loss', 'self_penetration_loss'):
            assert torch.equal(ld[k].detach(), base[k]), k
    fit.optimizer.step()
    assert torch.isfinite(fit.body_model.transl).all() and not torch.equal(fit.body_model.transl.detach(), t0)
    assert not torch.equal(count, find_collisions(verts, faces, max_pairs=2048, return_count=True, _lib=lib)[1]), 'the segmentation removes pairs'
    # the two marker terms
    sm = plain
    sm.w.update(smooth_vel_weight=3.0, smooth_acc_weight=5.0)
    with torch.no_grad():
        ld = sm.loss_dict()
    rv, ra = smooth_reference(host(verts)[:, np.asarray(prob['ids']['markers81'])], 3.0, 5.0)
    print(f'smooth_vel {float(ld["smooth_vel_loss"]):.8g} vs {rv:.8g}; smooth_acc {float(ld["smooth_acc_loss"]):.8g} vs {ra:.8g}')
    assert abs(float(ld['smooth_vel_loss']) - rv) <= 1e-5 * rv and abs(float(ld['smooth_acc_loss']) - ra) <= 1e-5 * ra and rv > 0 and ra > 0
    assert torch.equal(ld['total_loss'], (base['total_loss'] + ld['smooth_acc_loss']) + ld['smooth_vel_loss'])
    for k in base:
        if k not in ('total_loss', 'smooth_vel_loss', 'smooth_acc_loss'):
            assert torch.equal(ld[k].detach(), base[k]), k
    with pytest.raises(ValueError):
        fitter(selfpen=dict(height=1.0), faces_parents=parents)
    monkeypatch.undo()


def SYN_PARENTS():
    from lemo_amd import synthetic
    return synthetic.SMPLX_PARENTS.copy()


def check_fitter_graph(lib, device, monkeypatch):
    """GPU only: step(6, use_graph=True) against six eager steps.  The two runs take the same kernels in the same order; the only
    freedom is the order of the fp32 atomic adds of the scatter kernels (this term's and the chamfer family's), so the comparison is
    the project's loss-scalar tolerance, 1e-5 relative, after six steps."""
    prob, fitter, posed, faces = _fitter_setup(lib, device, monkeypatch)
    out = []
    for use_graph in (False, True):
        fit = fitter(selfpen=dict(sigma=0.5, max_pairs=2048))
        fit.w['coll_loss_weight'] = 0.01
        ld = fit.step(6, use_graph=use_graph)
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in ld.items()})
    a, b = out[0]['self_penetration_loss'], out[1]['self_penetration_loss']
    print(f'six steps: eager {a:.8g}, graph {b:.8g}, rel {abs(a - b) / a:.2e}')
    assert a > 0 and np.isfinite(b) and abs(a - b) <= 1e-5 * a
    monkeypatch.undo()


# ------------------------------------------------------------------------------------------------------------ full size
def pushed_body(lib, device, pushes=(0.55, 0.95)):
    """the synthetic body model with coherent skinning (V = 10475), posed, a surface-sized mesh of F = 20908 triangles over the posed
    cloud, and one frame per entry of ``pushes``: the arm vertices moved that share of the way to the torso -> (verts, faces)"""
    from lemo_amd import synthetic
    import __graft_entry__ as G
    prob = G.prox_small_problem(B=2, V=10475, coherent=True)
    fit = G.prox_fitter_for(prob, device, lib=lib)[0]
    with torch.no_grad():
        body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(2, -1)
        v0 = host(fit.body_model(return_verts=True, body_pose=body_pose).vertices[0]).astype(F64)
    faces = synthetic.local_faces(v0, 20908).astype(np.int64)
    dom = np.argmax(prob['model']['weights'], axis=1)
    arms, torso = np.isin(dom, (16, 17, 18, 19, 20, 21)), np.isin(dom, (3, 6, 9))
    shift = v0[torso].mean(0) - v0[arms].mean(0)
    frames = []
    for k, push in enumerate(pushes):
        v = v0.copy()
        v[arms] += shift * push
        frames.append(v + np.array([0.03 * k, -0.02 * k, 0.04 * k]))
    return dev(np.stack(frames), device, F32), faces


def check_full_size(lib, device):
    """GPU only: V = 10475, F = 20908, B = 2"""
    verts, faces = pushed_body(lib, device)
    assert tuple(verts.shape) == (2, 10475, 3) and faces.shape == (20908, 3)
    C = 1 << 17
    brute = find_collisions(verts, faces, max_pairs=C, mode='brute', return_count=True, _lib=lib)
    for kw in (dict(mode='grid'), dict(mode='grid', grid=8), dict(mode='auto')):
        got = find_collisions(verts, faces, max_pairs=C, return_count=True, _lib=lib, **kw)
        assert torch.equal(got[0], brute[0]) and torch.equal(got[1], brute[1]), kw
    lists = pair_sets(*brute)
    assert int(brute[1].max()) <= C
    sub = np.arange(0, 20908, 20908 // 512)[:512]
    vh = host(verts)
    for b in range(2):
        strict, loose, plain = collide64_subset(vh[b], faces, sub)
        got = {p for p in lists[b] if p[0] in set(sub.tolist()) or p[1] in set(sub.tolist())}
        excused = strict ^ loose
        print(f'full size frame {b}: {int(brute[1][b])} pairs, {len(plain)} float64 pairs at the 512 faces, excused {len(excused)}')
        assert len(plain) >= MIN_PAIRS and len(excused) <= EXCUSE_CAP * len(plain)
        assert not ((got ^ plain) - excused)


def collide64_subset(v, f, sub):
    """collide64 for the pairs with at least one face in ``sub``, against all faces"""
    lo, hi = _boxes(v[f], F64)
    ii, jj = [], []
    for s in sub:
        ov = np.all((lo[s] - 1e-3 <= hi) & (lo - 1e-3 <= hi[s]), axis=1) & ~(f[:, :, None] == f[s][None, None, :]).any((1, 2))
        for o in np.nonzero(ov)[0]:
            ii.append(min(s, o)); jj.append(max(s, o))
    i, j = np.array(ii, np.int64), np.array(jj, np.int64)
    A, Bt = v.astype(F64)[f[i]], v.astype(F64)[f[j]]
    hit = [np.zeros(len(i), bool) for _ in range(3)]
    for P, Q in ((A, Bt), (Bt, A)):
        for k in range(3):
            for n, h in enumerate(_seg_tri64(P[:, k], P[:, (k + 1) % 3], Q[:, 0], Q[:, 1], Q[:, 2], (SP_EPS, -SP_EPS, 0.0))):
                hit[n] |= h
    return [set(zip(i[h].tolist(), j[h].tolist())) for h in hit]


# ------------------------------------------------------------------------------------------------------------ compat, validation
def check_compat(lib, device, monkeypatch):
    import lemo_amd.compat as compat
    import lemo_amd.compat.mesh_intersection as mi
    monkeypatch.setattr(mi, '_lib', lib)
    names = ('mesh_intersection', 'mesh_intersection.bvh_search_tree', 'mesh_intersection.loss', 'mesh_intersection.filter_faces')
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        compat.install()
        from mesh_intersection.bvh_search_tree import BVH
        import mesh_intersection.loss as collisions_loss
        from mesh_intersection.filter_faces import FilterFaces
        verts, f = sp_case('spheres', 3)
        segm, parents = three_part_segmentation()
        v = dev(verts, device).requires_grad_(True)
        ft = dev(f, device, np.int64)
        triangles = torch.index_select(v, 1, ft.reshape(-1)).view(3, -1, 3, 3)             # fitting_temp_slide.py:623-625
        search_tree = BVH(max_collisions=8)
        pen = collisions_loss.DistanceFieldPenetrationLoss(sigma=0.5, point2plane=False, vectorized=True, penalize_outside=True)
        filt = FilterFaces(faces_segm=segm, faces_parents=parents, ign_part_pairs=['0,2']).to(device=device)
        with torch.no_grad():
            idx = search_tree(triangles).detach()
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (3, len(f) * 8, 2)
        pairs, count = find_collisions(dev(verts, device), f, max_pairs=len(f) * 8, return_count=True, _lib=lib)
        assert torch.equal(idx, pairs.long())
        for i in range(3):
            idx[i:i + 1] = filt(idx[i:i + 1])                                              # :630-632
        fp, fc = find_collisions(dev(verts, device), f, segm, parents, ['0,2'], max_pairs=len(f) * 8, return_count=True, _lib=lib)
        assert torch.equal(idx, fp.long()) and int(fc.min()) >= 1 and int((fc < count).sum()) == 3
        L = pen(triangles, idx)
        v2 = dev(verts, device).requires_grad_(True)
        L2 = penetration_loss(v2, f, fp, fc, 0.5, _lib=lib)
        assert torch.equal(L.detach(), L2.detach())
        L.sum().backward(); L2.sum().backward()
        scale = float(v2.grad.abs().max())
        assert scale > 0 and float((v.grad - v2.grad).abs().max()) <= 1e-5 * scale       # the same terms, scattered in another order
        with pytest.raises(NotImplementedError):
            collisions_loss.DistanceFieldPenetrationLoss(sigma=0.5, point2plane=True)
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
        monkeypatch.undo()


def check_validation(lib, device, monkeypatch):
    launched = []
    for name in SP_ENTRIES:
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    verts, f = sp_case('spheres', 3)
    B, V, F = verts.shape[0], verts.shape[1], len(f)
    v = dev(verts, device)
    segm = np.zeros(F, np.int32)
    E = (ValueError, _hip.LemoHipError)
    for kw in (dict(vertices=v.double()), dict(vertices=v[0]), dict(vertices=host(v)), dict(faces=f.astype(F64)), dict(faces=f[:, :2]),
               dict(faces=np.concatenate([f, [[0, 1, V]]])), dict(faces=dev(f, device, np.int64)), dict(mode='tree'), dict(grid=1), dict(grid=17),
               dict(max_pairs=0), dict(faces_segm=segm[:-1]), dict(faces_segm=segm.astype(F32)), dict(faces_parents=segm), dict(ign_part_pairs=['0,1']),
               dict(faces_segm=segm, ign_part_pairs=['0,64']), dict(faces_segm=segm, ign_part_pairs=np.zeros((65, 65), np.uint8)),
               dict(faces_segm=segm, ign_part_pairs=np.zeros((3, 4), np.uint8)), dict(faces_segm=dev(segm, device, np.int64))):
        args = dict(vertices=v, faces=f, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            find_collisions(**args)
    pr = torch.full((B, 4, 2), -1, dtype=torch.int32, device=device)
    cnt = torch.zeros(B, dtype=torch.int32, device=device)
    for kw in (dict(vertices=v.half()), dict(pairs=pr.long()), dict(pairs=pr[:2]), dict(pairs=pr[..., :1]), dict(pairs=host(pr)), dict(count=cnt.long()),
               dict(count=cnt[:2]), dict(count=host(cnt)), dict(sigma=0.0), dict(sigma=float('nan')), dict(sigma=torch.tensor(0.5))):
        args = dict(vertices=v, faces=f, pairs=pr, count=cnt, sigma=0.5, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            penetration_loss(**args)
    for kw in (dict(weight=-1.0), dict(weight=torch.tensor(1.0)), dict(sigma=0.0)):
        args = dict(vertices=v, faces=f, weight=1.0, _lib=lib)
        args.update(kw)
        with pytest.raises(E):
            self_penetration_term(**args)
    assert float(self_penetration_term(v, f, 0.0, _lib=lib)) == 0.0                    # a zero weight launches nothing
    if device.type != 'cpu':
        with pytest.raises(E):
            find_collisions(v.cpu(), f, _lib=lib)
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch
    S, A = 10001, 10002
    wsb = lib.selfpen_search_workspace_bytes
    assert wsb(1, 0, 1, 0, 0) == -1 and wsb(0, 1, 1, 0, 0) == -1 and wsb(1, 1, 1, 3, 0) == -1 and wsb(1, 1, 1, 0, 17) == -1 and wsb(1, 1, 1, 0, 1) == -1
    assert wsb(2, 10, 5, 1, 0) == 2 * 4 * 10 and wsb(2, 10, 5, 2, 4) == 2 * 4 * (10 + 16 + 64 + 1 + 35)
    se = lambda B=1, V=1, F=1, P=0, mode=1, grid=0, C=1, x=1, segm=None, par=None, ign=None, ws=1, wsb=1 << 20: \
        lib.selfpen_search(x, B, V, 1, F, segm, par, ign, P, mode, grid, 1, C, 1, ws, wsb, None)
    assert se(B=0) == S and se(V=0) == S and se(F=0) == S and se(C=0) == S and se(B=65536) == S
    assert se(mode=3) == A and se(grid=1) == A and se(grid=17) == A and se(x=None) == A and se(ws=None) == A and se(wsb=4) == A
    assert se(P=65, segm=1, ign=1) == A and se(P=2) == A and se(ign=1, segm=1) == A and se(par=1) == A and se(ign=1, P=2) == A
    lf = lambda B=1, V=1, F=1, C=1, sigma=0.5, x=1, out=1: lib.selfpen_loss_forward(x, B, V, 1, F, 1, C, None, sigma, 1, out, None)
    assert lf(B=0) == S and lf(C=0) == S and lf(sigma=0.0) == A and lf(sigma=float('nan')) == A and lf(x=None) == A and lf(out=None) == A
    lb = lambda B=1, C=1, sigma=0.5, g=1, out=1: lib.selfpen_loss_backward(1, B, 1, 1, 1, 1, C, None, sigma, 1, g, out, None)
    assert lb(B=0) == S and lb(sigma=-1.0) == A and lb(g=None) == A and lb(out=None) == A
