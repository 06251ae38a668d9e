"""Cases and yardsticks for lemo_amd.chamfer (csrc/chamfer_kernels.hip), shared by tests/test_chamfer_emu.py (host emulator) and
tests/test_chamfer_gpu.py (MI355X).

The yardstick is a numpy restatement written for these tests: all-pairs squared distances in int64 (lattice points: exact, ties
everywhere, numpy's first-occurrence argmin) or float64 on the same float32 inputs.  Tolerances are derived, not fitted:

* forward: ``|dist - d64[idx]| <= 6 * 2^-24 * d64[idx]`` -- one rounding in each difference (entering twice through the square), one per
  square and one per addition, with the margin for the unfused order; ``d64[idx] <= (1 + 12 * 2^-24) * min d64`` -- the chosen target
  is a nearest one up to twice that rounding.
* backward: per element ``4 K 2^-24 sum|terms|`` with K the number of terms that land on it and the sum taken in float64 -- two
  roundings per term (difference, product; the factor 2 g is exact) and K - 1 roundings of partial sums that never exceed sum|terms|.
* contact term: 1e-5 relative for the loss scalar and its gradient (the project's loss-scalar tolerance).
"""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest
import torch

from lemo_amd import _hip
from lemo_amd import chamfer as CH
from lemo_amd.chamfer import ChamferDist, chamfer_distance, contact_term

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_Q, _C, _S = CH.QUERIES_PER_WORKGROUP, CH.LDS_CHUNK, CH.SPLIT_LENGTH
# (B, N, M): the issue's four, then one below / at / above the queries of a workgroup (N; the reverse direction puts the same sizes on
# the target side), the LDS chunk, the split length, and twice the split length (the first M the automatic rule cuts in two)
LATTICE_SHAPES = [(1, 1, 1), (2, 7, 5), (1, 65, 257), (3, 300, 1030)] + \
    [(1, _Q + k, 3) for k in (-1, 0, 1)] + [(2, 3, _C + k) for k in (-1, 0, 1)] + [(1, 5, _S + k) for k in (-1, 0, 1)] + \
    [(1, 5, 2 * _S + k) for k in (-1, 0, 1)]
RANDOM_SHAPES = [(2, 70, 130), (1, 300, 2 * _S + 7)]
RANDOM_KINDS = ['normal', 'prox']


def dev(a, device, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(device)          # a copy: the cached cases are read-only


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def lattice_case(B, N, M):
    rng = np.random.default_rng(1000 * B + 10 * N + M)
    a, b = rng.integers(-4, 5, (B, N, 3)), rng.integers(-4, 5, (B, M, 3))
    D = ((a[:, :, None, :] - b[:, None, :, :]).astype(np.int64) ** 2).sum(-1)            # [B, N, M] exact
    ref = (D.min(2), D.min(1), D.argmin(2), D.argmin(1))
    for r in (a, b) + ref:
        r.setflags(write=False)
    return a.astype(F32), b.astype(F32), ref


@functools.lru_cache(maxsize=None)
def random_case(B, N, M, kind):
    rng = np.random.default_rng(7 + 1000 * B + 10 * N + M)
    a, b = rng.standard_normal((B, N, 3)), rng.standard_normal((B, M, 3))
    if kind == 'prox':                                            # metres: a body-sized cloud in a room, away from the origin
        a, b = 0.8 * a + 3.0, 1.5 * b + 3.0
    a, b = a.astype(F32), b.astype(F32)
    d = a.astype(F64)[:, :, None, :] - b.astype(F64)[:, None, :, :]
    D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]           # [B, N, M] float64 on the float32 inputs
    for r in (a, b, D):
        r.setflags(write=False)
    return a, b, D


def check_sizes(lib):
    """the constants the cases are built from are the library's"""
    assert CH.library_sizes(lib) == (CH.QUERIES_PER_WORKGROUP, CH.LDS_CHUNK, CH.SPLIT_LENGTH, CH.SPLIT_TARGET_WORKGROUPS)


# ------------------------------------------------------------------------------------------------------------ 1. exact lattice
def check_lattice(lib, device, B, N, M):
    a, b, (d1, d2, i1, i2) = lattice_case(B, N, M)
    o1, o2, j1, j2 = chamfer_distance(dev(a, device), dev(b, device), _lib=lib)
    assert o1.dtype == torch.float32 and j1.dtype == torch.int32 and tuple(o1.shape) == (B, N) and tuple(j2.shape) == (B, M)
    assert np.array_equal(host(o1).astype(np.int64), d1) and np.array_equal(host(o1), d1.astype(F32))
    assert np.array_equal(host(o2).astype(np.int64), d2) and np.array_equal(host(o2), d2.astype(F32))
    assert np.array_equal(host(j1), i1), 'idx1 is not the first-occurrence argmin'
    assert np.array_equal(host(j2), i2), 'idx2 is not the first-occurrence argmin'


# ------------------------------------------------------------------------------------------------------------ 2. random points
def _check_forward(dist, idx, D, what):
    """dist, idx [B, N] against all-pairs float64 D [B, N, M]; every element takes part in both bounds"""
    assert idx.min() >= 0 and idx.max() < D.shape[2]
    at = np.take_along_axis(D, idx[..., None].astype(np.int64), 2)[..., 0]
    e1 = np.abs(dist.astype(F64) - at) / np.maximum(at, 1e-300)
    e2 = at / np.maximum(D.min(2), 1e-300) - 1.0
    print(f'{what}: |dist - d64[idx]| / d64[idx] max {e1.max() / EPS:.2f} x 2^-24 (bound 6); d64[idx] / min d64 - 1 max '
          f'{e2.max() / EPS:.2f} x 2^-24 (bound 12)')
    assert np.all(np.abs(dist.astype(F64) - at) <= 6 * EPS * at), what
    assert np.all(at <= (1 + 12 * EPS) * D.min(2)), what


def check_random(lib, device, B, N, M, kind):
    a, b, D = random_case(B, N, M, kind)
    o1, o2, j1, j2 = chamfer_distance(dev(a, device), dev(b, device), _lib=lib)
    _check_forward(host(o1), host(j1), D, f'{kind} ({B}, {N}, {M}) dist1')
    _check_forward(host(o2), host(j2), D.transpose(0, 2, 1), f'{kind} ({B}, {N}, {M}) dist2')


# ------------------------------------------------------------------------------------------------------------ 3. independence
def _same(x, y):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(x, y))


def check_independence(lib, device):
    B, N, M = 3, 33, 2 * _S + 7
    a, b, _ = random_case(B, N, M, 'normal')
    A, Bt = dev(a, device), dev(b, device)
    base = chamfer_distance(A, Bt, _lib=lib)
    assert _same(base, chamfer_distance(A, Bt, _lib=lib)), 'two runs differ'
    for split in (1, 2, 7):
        assert _same(base, chamfer_distance(A, Bt, split=split, _lib=lib)), f'split override {split} changes the result'
        ws = lib.chamfer_workspace_bytes(B, N, M, CH.REVERSE, split)
        assert (ws == 0) == (split == 1), (split, ws)                     # the overrides really take the split path
    one = chamfer_distance(A, Bt, bidirectional=False, _lib=lib)
    assert one[1] is None and one[3] is None and torch.equal(one[0], base[0]) and torch.equal(one[2], base[2])
    # lattice ties across split boundaries: every split holds copies of the same points
    la, lb, (d1, _, i1, _) = lattice_case(3, 300, 1030)
    for split in (1, 2, 7):
        o1, _, j1, _ = chamfer_distance(dev(la, device), dev(lb, device), bidirectional=False, split=split, _lib=lib)
        assert np.array_equal(host(o1), d1.astype(F32)) and np.array_equal(host(j1), i1), split
    # one shared target against the same target repeated
    shared = chamfer_distance(A, Bt[:1].contiguous(), bidirectional=False, _lib=lib)
    rep = chamfer_distance(A, Bt[:1].repeat(B, 1, 1), bidirectional=False, _lib=lib)
    assert _same(shared, rep), 'a shared target differs from the repeated one'
    for split in (2, 7):
        assert _same(shared, chamfer_distance(A, Bt[:1].contiguous(), bidirectional=False, split=split, _lib=lib))


# ------------------------------------------------------------------------------------------------------------ 4. backward
def backward_reference(a, b, g1, i1, g2, i2):
    """float64 gradients for the given indices, with per-element (K, sum|terms|); b may be [1, M, 3] (shared: summed over the batch)"""
    a64, b64 = a.astype(F64), b.astype(F64)
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    shared = b.shape[0] == 1 and B > 1
    G = [np.zeros((B, N, 3)), np.zeros(b64.shape)]
    S = [np.zeros((B, N, 3)), np.zeros(b64.shape)]
    K = [np.zeros((B, N)), np.zeros(b64.shape[:2])]
    for bb in range(B):
        tb = 0 if shared else bb
        t = 2.0 * g1[bb].astype(F64)[:, None] * (a64[bb] - b64[tb][i1[bb]])                # [N, 3]: own term of side 1
        G[0][bb] += t; S[0][bb] += np.abs(t); K[0][bb] += 1
        np.add.at(G[1][tb], i1[bb], -t); np.add.at(S[1][tb], i1[bb], np.abs(t)); np.add.at(K[1][tb], i1[bb], 1)
        if g2 is not None:
            u = 2.0 * g2[bb].astype(F64)[:, None] * (b64[bb] - a64[bb][i2[bb]])            # [M, 3]: own term of side 2
            G[1][bb] += u; S[1][bb] += np.abs(u); K[1][bb] += 1
            np.add.at(G[0][bb], i2[bb], -u); np.add.at(S[0][bb], i2[bb], np.abs(u)); np.add.at(K[0][bb], i2[bb], 1)
    return G, S, K


def _check_grad(got, G, S, K, what):
    bound = 4 * K[..., None] * EPS * S
    err = np.abs(got.astype(F64) - G)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{what}: worst error / bound {ratio:.3f}, K up to {int(K.max())}')
    assert np.all(err <= bound), what


class _Recorder:
    """wraps an entry of the library: counts the calls and keeps the last argument list"""

    def __init__(self, fn):
        self.fn, self.calls, self.args = fn, 0, None

    def __call__(self, *a):
        self.calls += 1
        self.args = a
        return self.fn(*a)


def check_backward(lib, device, monkeypatch, B, N, M, kind, bidirectional=True, shared=False):
    a, b, _ = random_case(B, N, M, kind)
    if shared:
        b = b[:1]
    rng = np.random.default_rng(B + N + M)
    g1 = rng.standard_normal((B, N)).astype(F32)
    g2 = rng.standard_normal((B, M)).astype(F32) if bidirectional else None
    rec = _Recorder(lib.chamfer_backward)
    monkeypatch.setattr(lib, 'chamfer_backward', rec)
    for need1, need2 in ((True, True), (True, False), (False, True)):
        A, Bt = dev(a, device).requires_grad_(need1), dev(b, device).requires_grad_(need2)
        d1, d2, i1, i2 = chamfer_distance(A, Bt, bidirectional=bidirectional, _lib=lib)
        assert not i1.requires_grad and d1.requires_grad
        loss = (d1 * dev(g1, device)).sum() + ((d2 * dev(g2, device)).sum() if bidirectional else 0.0)
        calls = rec.calls
        loss.backward()
        assert rec.calls == calls + 1
        # argument list of lemo_chamfer_backward: ..., grad1, grad2, stream -- a side that is not needed gets no buffer at all
        assert (rec.args[-3] is not None) == need1 and (rec.args[-2] is not None) == need2
        assert (A.grad is not None) == need1 and (Bt.grad is not None) == need2
        G, S, K = backward_reference(a, b, g1, host(i1), g2, None if i2 is None else host(i2))
        tag = f'{kind} ({B}, {N}, {M}) bidirectional={bidirectional} shared={shared}'
        if need1:
            assert tuple(A.grad.shape) == (B, N, 3)
            _check_grad(host(A.grad), G[0], S[0], K[0], tag + ' grad1')
        if need2:
            assert tuple(Bt.grad.shape) == tuple(b.shape)
            _check_grad(host(Bt.grad), G[1], S[1], K[1], tag + ' grad2')
            if not bidirectional:
                assert np.all(host(Bt.grad)[K[1] == 0] == 0.0), 'a target nobody chose has a gradient'
    monkeypatch.undo()


def check_module_backward(lib, device):
    """ChamferDist (the reference's chamferDist call shape) through torch.autograd.backward"""
    B, N, M = 2, 70, 130
    a, b, _ = random_case(B, N, M, 'prox')
    rng = np.random.default_rng(5)
    g1, g2 = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, M)).astype(F32)
    A, Bt = dev(a, device).requires_grad_(True), dev(b, device).requires_grad_(True)
    d1, d2, i1, i2 = ChamferDist(_lib=lib)(A, Bt)
    torch.autograd.backward([d1, d2], [dev(g1, device), dev(g2, device)])
    G, S, K = backward_reference(a, b, g1, host(i1), g2, host(i2))
    _check_grad(host(A.grad), G[0], S[0], K[0], 'ChamferDist grad1')
    _check_grad(host(Bt.grad), G[1], S[1], K[1], 'ChamferDist grad2')


# ------------------------------------------------------------------------------------------------------------ 5. compat
def check_compat(lib, device, monkeypatch):
    """chamfer.forward / backward with the buffers temp_prox/dist_chamfer.py:16-25, 37-41 allocates: zeros, int32 indices"""
    import lemo_amd.compat.chamfer as cc
    monkeypatch.setattr(cc, '_lib', lib)
    B, N, M = 2, 70, 130
    a, b, D = random_case(B, N, M, 'prox')
    A, Bt = dev(a, device), dev(b, device)
    dist1, dist2 = torch.zeros(B, N, device=device), torch.zeros(B, M, device=device)
    idx1, idx2 = torch.zeros(B, N, device=device).type(torch.int32), torch.zeros(B, M, device=device).type(torch.int32)
    cc.forward(A, Bt, dist1, dist2, idx1, idx2)
    want = chamfer_distance(A, Bt, _lib=lib)
    assert _same((dist1, dist2, idx1, idx2), want)
    _check_forward(host(dist1), host(idx1), D, 'compat dist1')
    _check_forward(host(dist2), host(idx2), D.transpose(0, 2, 1), 'compat dist2')
    rng = np.random.default_rng(6)
    g1, g2 = rng.standard_normal((B, N)).astype(F32), rng.standard_normal((B, M)).astype(F32)
    gx1, gx2 = torch.zeros(A.size(), device=device), torch.zeros(Bt.size(), device=device)
    cc.backward(A, Bt, gx1, gx2, dev(g1, device), dev(g2, device), idx1, idx2)
    G, S, K = backward_reference(a, b, g1, host(idx1), g2, host(idx2))
    _check_grad(host(gx1), G[0], S[0], K[0], 'compat gradxyz1')
    _check_grad(host(gx2), G[1], S[1], K[1], 'compat gradxyz2')
    # anything that is not a device tensor: no CPU path
    with pytest.raises(NotImplementedError):
        cc.forward(None, None, None, None, None, None)
    with pytest.raises(NotImplementedError):
        cc.forward(a, b, host(dist1), host(dist2), host(idx1), host(idx2))
    with pytest.raises(NotImplementedError):
        cc.backward(A, Bt, gx1, gx2, g1, g2, idx1, idx2)
    if device.type != 'cpu':
        with pytest.raises(NotImplementedError):
            cc.forward(A.cpu(), Bt.cpu(), dist1.cpu(), dist2.cpu(), idx1.cpu(), idx2.cpu())
    monkeypatch.undo()


def check_compat_without_a_library():
    """the module as LEMO imports it (no test library installed): CPU tensors and None are refused, nothing is loaded"""
    import lemo_amd.compat.chamfer as cc
    assert cc._lib is None
    z = torch.zeros(1, 2, 3)
    with pytest.raises(NotImplementedError, match='no CPU path'):
        cc.forward(z, z, torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        cc.backward(None, None, None, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------------------ 6. contact term
def contact_reference(vw, ids, scene, weight):
    """float64 value and gradient of fitting_temp_slide.py:743-753 on the float32 inputs"""
    v = torch.from_numpy(vw.astype(F64)).requires_grad_(True)
    s = torch.from_numpy(scene.astype(F64))
    body = v[:, torch.from_numpy(np.asarray(ids, np.int64)), :]
    d = ((body[:, :, None, :] - s[None, None, :, :]) ** 2).sum(-1).min(2).values
    r = torch.sqrt(d + 1e-4)
    loss = weight * (r / (r + 1.0)).mean()
    loss.backward()
    return float(loss.detach()), v.grad.numpy()


def check_contact_term(lib, device, B):
    rng = np.random.default_rng(40 + B)
    V, P, M = 60, 40, 500
    scene = (rng.random((M, 3)) * np.array([4.0, 4.0, 0.05]) + np.array([1.0, 1.0, 1.4])).astype(F32)      # a rough floor
    vw = (rng.standard_normal((B, V, 3)) * 0.4 + np.array([3.0, 3.0, 1.8])).astype(F32)
    ids = rng.permutation(V)[:P]
    on = rng.permutation(P)[:8]                                   # 8 contact points per frame lie ON scene vertices: d = 0
    for bb in range(B):
        vw[bb, ids[on]] = scene[rng.integers(0, M, 8)]
    weight = 1.7
    want, gwant = contact_reference(vw, ids, scene, weight)
    for scene_t in (dev(scene, device), dev(scene[None], device)):
        v = dev(vw, device).requires_grad_(True)
        loss = contact_term(v, ids, scene_t, weight, _lib=lib)
        loss.backward()
        e = abs(float(loss.detach()) - want) / abs(want)
        g = host(v.grad)
        ge = float(np.abs(g - gwant).max() / np.abs(gwant).max())
        print(f'contact_term B = {B}: value rel {e:.2e}, gradient rel {ge:.2e} (bound 1e-5)')
        assert e <= 1e-5 and ge <= 1e-5
        assert np.isfinite(g).all() and np.all(g[:, np.setdiff1d(np.arange(V), ids)] == 0.0)
        d, _, _, _ = chamfer_distance(v.detach()[:, dev(ids, device, np.int64)].contiguous(), dev(scene[None], device), False, _lib=lib)
        assert int((d == 0).sum()) >= 8 * B                        # the 1e-4 under the root matters here


def floor_and_box_scene():
    """world coordinates of __graft_entry__.prox_small_problem: the floor plane z = 1.40 the synthetic SDF has, and a box on it"""
    g = np.arange(-3.0, 3.0001, 0.1)
    fx, fy = np.meshgrid(g, g, indexing='ij')
    floor = np.stack([fx.ravel(), fy.ravel(), np.full(fx.size, 1.40)], -1)
    u = np.arange(0.0, 0.5001, 0.05)
    bx, by, bz = np.meshgrid(0.3 + u, -2.2 + u, 1.40 + u, indexing='ij')
    box = np.stack([bx.ravel(), by.ravel(), bz.ravel()], -1)
    shell = (np.isclose(box[:, 0], 0.3) | np.isclose(box[:, 0], 0.8) | np.isclose(box[:, 1], -2.2) | np.isclose(box[:, 1], -1.7) |
             np.isclose(box[:, 2], 1.90))
    return np.concatenate([floor, box[shell]]).astype(F32)


def golden_contact_ids():
    ids = np.load(os.path.join(GOLDEN, 'contact_verts_ids.npz'))['contact_verts_ids']
    assert ids.shape == (1121,) and len(set(ids.tolist())) == 1121 and ids[0] == 5774          # CPython set order, not sorted
    return ids


def check_prox_fitter(lib, device, monkeypatch):
    """ProxTemporalFitter with a scene: B = 14 frames of the SMPL-X-sized synthetic body (the golden ids reach vertex 8934)"""
    import __graft_entry__ as G
    from lemo_amd.prox import ProxTemporalFitter                    # noqa: F401
    prob = G.prox_small_problem(B=14, V=10475)
    ids, scene = golden_contact_ids(), dev(floor_and_box_scene(), device)
    rec = _Recorder(lib.chamfer_forward)
    monkeypatch.setattr(lib, 'chamfer_forward', rec)

    def fitter(**kw):
        import lemo_amd.prox as P
        real = P.ProxTemporalFitter
        monkeypatch.setattr(P, 'ProxTemporalFitter', lambda *a, **k: real(*a, **k, **kw))
        try:
            return G.prox_fitter_for(prob, device, lib=lib)[0]
        finally:
            monkeypatch.setattr(P, 'ProxTemporalFitter', real)

    def same(ld, base):
        return set(ld) == set(base) and all(torch.equal(ld[k].detach(), base[k]) for k in base)

    assert 'contact_loss_weight' not in prob['weights']
    plain = fitter()                                                # the fitter as it was: no new argument, no new weight
    base = {k: v.detach().clone() for k, v in plain.closure().items()}
    g0 = plain.pose_embedding.grad.detach().clone()
    assert float(base['contact_loss']) == 0.0
    plain.w['contact_loss_weight'] = 1.0                            # a weight without a scene
    with torch.no_grad():
        assert same(plain.loss_dict(), base)
    fit = fitter(scene_v=scene, contact_verts_ids=ids)
    with torch.no_grad():
        assert same(fit.loss_dict(), base)                          # a scene without a weight
        fit.w['contact_loss_weight'] = 0.0
        assert same(fit.loss_dict(), base)
    assert rec.calls == 0, 'the contact term was launched without scene, ids or weight'
    fit.w['contact_loss_weight'] = 1.0
    ld = fit.closure()
    assert rec.calls == 1
    c = ld['contact_loss'].detach()
    print(f'PROX window B = 14: contact_loss {float(c):.6f}, total {float(base["total_loss"]):.6f} -> {float(ld["total_loss"]):.6f}')
    assert float(c) > 0
    assert torch.equal(ld['total_loss'].detach(), base['total_loss'] + c), 'total_loss does not rise by exactly the contact term'
    for k in base:
        if k not in ('total_loss', 'contact_loss'):
            assert torch.equal(ld[k].detach(), base[k]), k
    g1 = fit.pose_embedding.grad
    assert torch.isfinite(g1).all() and not torch.equal(g1, g0)
    erase = int(14 * 0.15)
    assert float((g1[erase:] - g0[erase:]).abs().max()) > 0
    monkeypatch.undo()


# ------------------------------------------------------------------------------------------------------------ 7. validation
def check_validation(lib, device, monkeypatch):
    launched = []
    for name in ('chamfer_forward', 'chamfer_backward'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    a, b = torch.zeros(2, 7, 3, device=device), torch.zeros(2, 5, 3, device=device)
    other = torch.device('cpu') if device.type != 'cpu' else None
    bad = [dict(xyz1=a.double()), dict(xyz2=b.double()), dict(xyz1=a.half()), dict(xyz2=b.int()), dict(xyz1=a[0]), dict(xyz2=b[0]),
           dict(xyz1=a[..., :2]), dict(xyz2=b[..., :2]), dict(xyz1=a[:, :0]), dict(xyz2=b[:, :0]), dict(xyz1=a[:0], xyz2=b[:0]),
           dict(xyz2=torch.zeros(3, 5, 3, device=device)), dict(xyz1=a[:1]), dict(xyz2=b[:1]),            # the last: shared AND two-sided
           dict(xyz1=host(a)), dict(xyz2=host(b)), dict(xyz1=None), dict(split=-1)]
    if other is not None:
        bad += [dict(xyz1=a.to(other)), dict(xyz2=b.to(other)), dict(xyz1=a.to(other), xyz2=b.to(other))]
    for kw in bad:
        args = dict(xyz1=a, xyz2=b, _lib=lib)
        args.update(kw)
        with pytest.raises((ValueError, _hip.LemoHipError)):
            chamfer_distance(**args)
    with pytest.raises((ValueError, _hip.LemoHipError)):
        ChamferDist(_lib=lib)(a, b[:1])
    vw, scene = torch.zeros(2, 9, 3, device=device), torch.zeros(5, 3, device=device)
    for kw in (dict(contact_verts_ids=[0, 9]), dict(contact_verts_ids=[-1]), dict(contact_verts_ids=[]), dict(contact_verts_ids=[0.5]),
               dict(contact_verts_ids=[[0, 1]]), dict(scene_v=scene[:, :2]), dict(scene_v=torch.zeros(2, 5, 3, device=device)),
               dict(scene_v=host(scene)), dict(scene_v=scene.double()), dict(scene_v=scene[:0]), dict(vertices_world=vw[0]),
               dict(vertices_world=vw.double())):
        args = dict(vertices_world=vw, contact_verts_ids=[0, 3], scene_v=scene, weight=1.0, _lib=lib)
        args.update(kw)
        with pytest.raises((ValueError, _hip.LemoHipError)):
            contact_term(**args)
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own, before any launch (addresses are never dereferenced on these paths)
    f = lambda B=1, N=1, M=1, flags=0, split=0, x1=1, d2=None, ws=None, wsb=0: lib.chamfer_forward(
        x1, 1, B, N, M, flags, split, 1, 1, d2, d2, ws, wsb, None)
    assert f(N=0) == 10001 and f(M=0) == 10001 and f(B=0) == 10001 and f(B=65536) == 10001 and f(B=2, N=1 << 30) == 10001
    assert f(x1=None) == 10002 and f(flags=3) == 10002 and f(flags=4) == 10002 and f(flags=2) == 10002 and f(split=-1) == 10002
    assert f(M=4096, split=2) == 10002                                                           # a split without its workspace
    assert lib.chamfer_workspace_bytes(1, 0, 1, 0, 0) == -1 and lib.chamfer_workspace_bytes(2, 1, 1, 3, 0) == -1
    bw = lambda flags=0, g1=1, g2=None: lib.chamfer_backward(1, 1, 1, 1, 1, flags, g1, 1, g2, g2, None, None, None)
    assert bw() == 0 and bw(g1=None) == 10002 and bw(flags=2) == 10002 and bw(flags=3) == 10002


# ------------------------------------------------------------------------------------------------------------ 8. full size (GPU)
def check_full_size(lib, device):
    """the contact shape once: B = 100 frames x 1121 contact vertices against one shared scene of 200 000 vertices (an assumed size:
    no PROX scene mesh is part of this project), one-sided, forward and backward; float64 on a fixed sample of 2 000 queries"""
    B, N, M, nsample = 100, 1121, 200_000, 2000
    g = torch.Generator().manual_seed(11)
    scene = (torch.rand(M, 3, generator=g) * torch.tensor([6.0, 6.0, 2.5])).to(device)
    body = (torch.randn(B, N, 3, generator=g) * 0.4 + torch.tensor([3.0, 3.0, 1.0])).to(device).requires_grad_(True)
    gout = torch.randn(B, N, generator=g).to(device)
    torch.cuda.synchronize()
    chamfer_distance(body.detach(), scene[None], bidirectional=False, _lib=lib)                    # first launch: code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d, _, idx, _ = chamfer_distance(body, scene[None], bidirectional=False, _lib=lib)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    (d * gout).sum().backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'full size B = {B}, N = {N}, M = {M} (assumed scene size): forward {1e3 * (t1 - t0):.2f} ms = '
          f'{B * N * M / (t1 - t0) / 1e12:.2f} T pair-evaluations/s, backward {1e3 * (t2 - t1):.2f} ms (host clocks, one run, not gated)')
    sel = torch.randperm(B * N, generator=torch.Generator().manual_seed(3))[:nsample].to(device)
    q = body.detach().reshape(-1, 3)[sel].double()
    s64 = scene.double()
    at, mn = [], []
    for lo in range(0, nsample, 250):
        qq = q[lo:lo + 250]
        diff = [qq[:, c:c + 1] - s64[None, :, c] for c in range(3)]
        D = (diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]                            # [250, M] float64
        j = idx.reshape(-1)[sel[lo:lo + 250]].long()
        assert int(j.min()) >= 0 and int(j.max()) < M
        at.append(D.gather(1, j[:, None])[:, 0]); mn.append(D.min(1).values)
    at, mn = torch.cat(at), torch.cat(mn)
    ds = d.detach().reshape(-1)[sel].double()
    print(f'  |dist - d64[idx]| / d64[idx] max {float(((ds - at).abs() / at).max()) / EPS:.2f} x 2^-24 (bound 6); '
          f'd64[idx] / min d64 - 1 max {float((at / mn - 1).max()) / EPS:.2f} x 2^-24 (bound 12)')
    assert bool(((ds - at).abs() <= 6 * EPS * at).all()) and bool((at <= (1 + 12 * EPS) * mn).all())
    j = idx.reshape(-1)[sel].long()
    term = 2.0 * gout.reshape(-1)[sel].double()[:, None] * (q - s64[j])                           # K = 1: the own-side store
    err = (body.grad.reshape(-1, 3)[sel].double() - term).abs()
    assert bool((err <= 4 * EPS * term.abs()).all())
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(body.grad).all())
