"""Cases and yardsticks for the optional terms of the PROX window engine (lemo_prox_set_terms, csrc/prox_terms_kernels.hip: contact,
s2m / m2s, self-penetration, marker velocity / acceleration inside ``ProxWindowEngine``), shared by tests/test_prox_terms_emu.py (host
emulator) and tests/test_prox_terms_gpu.py (MI355X).

Every case is one window of B = 14 frames.  Contact, scan and velocity run on ``prox_small_problem(B=14, V=640)``, self-penetration
and the all-terms case on V = 10475 (the set-up of selfpen_common._fitter_setup), both with ``synthetic.local_faces`` for a
surface-sized mesh; one contact + velocity case runs on V = 10475 so that the chunked all-vertex backward sees the added gradient.
M = 300 scene vertices, S = 256 padded scan points, scan_point_num = 256 except 128, 37 and one 0 (a dropped frame).

Parity (engine against ``ProxTemporalFitter`` on the same device): the gates of tests/test_prox_engine_emu.py -- every LOSS_KEYS
entry within 1e-5 |ref| + 1e-12, every ENGINE_PARAMS gradient rel_err < 2e-4, parameters after one step within 2e-6.

Float64 (``terms_restated``): the six values and the terms' share of d(loss)/d(verts), restated in torch with autograd on the engine's
own vertices and decisions (nearest indices, visibility, collision pairs).  Tolerances follow selfpen_common's method: the SAME
restatement evaluated in float32 shows what fp32 arithmetic on these inputs loses against float64; the engine may lose 4 x that, with
a floor of 16 x 2^-24 (a dozen fp32 roundings per element; sums are taken in double on the device).  The measured share of the
gradient is the difference of two fp32 buffers (engine with the terms minus engine without, same vertices bit for bit), each entry of
which took at most 5 more fp32 additions at the magnitude of the full gradient: 5 x 2^-24 x max |dverts| is added to the bound.
The base engine of that difference runs with the S2 / S3 weights at 0, so that max |dverts| is the terms' own share.
Measured on the emulator (B = 14): values 3.1e-9 .. 4.3e-8 relative (bound 9.5e-7, the floor); gradient share 1.3e-6 (contact, bound
5.7e-6), 4.7e-8 (scan, bound 1.3e-6), 6.7e-8 (velocity, bound 1.3e-6), 1.1e-2 (self-penetration, bound 1.7e-1: on this window's
stretched triangles with up to 98000 pairs per frame the float32 restatement itself is 4.3e-2 away from float64; the engine's
fixed-point adjoint and lemo_selfpen_loss_backward's fp32-atomic one, which share every instruction but the accumulation, differ by
5.6e-7 of the largest entry on the same vertices and pairs).
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from chamfer_common import floor_and_box_scene, golden_contact_ids
from scan_common import body_mask_golden
from selfpen_common import SYN_PARENTS, _Recorder, loss64

F32, F64 = np.float32, np.float64
B, S, M = 14, 256, 300
EPS32 = 2.0 ** -24
SINGLE = ('contact', 'scan', 'selfpen', 'velocity')
BIG = {'contact': 640, 'scan': 640, 'velocity': 640, 'selfpen': 10475, 'all': 10475, 'contact_velocity_big': 10475, 'overflow': 10475}
PARITY_CASES = [(w, f) for w in SINGLE + ('all',) for f in (False, True)] + [('contact_velocity_big', False), ('overflow', False)]
WEIGHTS = dict(contact=dict(contact_loss_weight=1.0), scan=dict(s2m_weight=2.0, m2s_weight=3.0, rho_s2m=0.2, rho_m2s=0.1),
               selfpen=dict(coll_loss_weight=0.01), velocity=dict(smooth_vel_weight=3.0, smooth_acc_weight=5.0))
SELFPEN = dict(sigma=0.5, penalize_outside=True, max_pairs=131072)      # the window's frames hold up to ~98000 pairs (printed by the cases)
OVERFLOW_PAIRS = 2048                                                     # selfpen_common._fitter_setup's list: every frame but the first overflows
TERM_KEYS = dict(contact=('contact_loss',), scan=('s2m_dist', 'm2s_dist'), selfpen=('self_penetration_loss',),
                 velocity=('smooth_acc_loss', 'smooth_vel_loss'))


def host(t):
    return t.detach().cpu().numpy()


def parts_of(which):
    return {'all': SINGLE, 'contact_velocity_big': ('contact', 'velocity'), 'overflow': ('selfpen',)}.get(which, (which,))


# ------------------------------------------------------------------------------------------------------------ construction
def _modules(prob, device, lib, move):
    from lemo_amd.body_model import create
    from lemo_amd.priors import Enc
    from lemo_amd.vposer import VPoser
    bm = create(prob['model'], batch_size=prob['B'], extra_joint_ids=list(range(21)) if prob['V'] < 9930 else None, _lib=lib)
    vp = VPoser(_lib=lib).eval()
    vp.load_state_dict({**vp.state_dict(), **{k: torch.from_numpy(v) for k, v in prob['vposer_w'].items()}})
    enc = Enc(_lib=lib)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in prob['enc_w'].items()})
    if move:
        vp, enc = vp.to(device), enc.to(device)
    return bm.to(device), vp, enc


def _fresh(params):
    """the fitter's parameters may alias the arrays they were made from, and its optimiser writes in place: every object gets its own"""
    return {k: np.array(v, copy=True) for k, v in params.items()}


def fitter_for(prob, device, lib, first=False, **kw):
    """__graft_entry__.prox_fitter_for with the optional-term arguments"""
    from lemo_amd.prox import ProxTemporalFitter
    bm, vp, enc = _modules(prob, device, lib, True)
    return ProxTemporalFitter(bm, vp, enc, prob['ids'], prob['Xmean'], prob['Xstd'], prob['weights'], prob['R'], prob['t'],
                              torch.from_numpy(prob['sdf']).to(device), prob['grid_min'], prob['grid_max'], _fresh(prob['params']), prob['gt_joints'],
                              prob['joints_conf'], fric_ids=prob['fric_ids'], first_batch_flag=first, **prob['infill'], **kw)


def engine_for(prob, device, lib, first=False, **kw):
    """__graft_entry__.prox_engine_for with the optional-term arguments"""
    from lemo_amd.prox import ProxWindowEngine
    bm, vp, enc = _modules(prob, device, lib, False)
    return ProxWindowEngine(bm, vp, enc, prob['ids'], prob['Xmean'], prob['Xstd'], prob['weights'], prob['R'], prob['t'],
                            torch.from_numpy(prob['sdf']).to(device), prob['grid_min'], prob['grid_max'], _fresh(prob['params']), prob['gt_joints'],
                            prob['joints_conf'], joint_map=prob['joint_map'], fric_ids=prob['fric_ids'], first_batch_flag=first,
                            **prob['infill'], **kw)


_SETUPS = {}


def setup(lib, device, V):
    """the window, its mesh, scene, scan and segmentation; computed once per (library, device, V) and never modified"""
    key = (lib.path, str(device), V)
    if key in _SETUPS:
        return _SETUPS[key]
    import __graft_entry__ as G
    from lemo_amd import synthetic
    from lemo_amd.selfpen import segmentation_from_weights
    prob = G.prox_small_problem(B=B, V=V)
    fit = fitter_for(prob, device, lib)
    with torch.no_grad():
        body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(B, -1)
        verts = fit.body_model(return_verts=True, body_pose=body_pose).vertices.detach().contiguous()
    faces = synthetic.local_faces(host(verts)[0], 1200)
    prob['model'] = dict(prob['model'], f=faces)
    rng = np.random.default_rng(11)
    scene = floor_and_box_scene()
    scene = scene[rng.permutation(len(scene))[:M]]
    ids = golden_contact_ids() if V == 10475 else rng.permutation(V)[:48]
    pick = rng.integers(0, V, (B, S))
    scan = np.take_along_axis(host(verts), pick[..., None], 1) + rng.normal(0, 0.02, (B, S, 3))
    spn = np.full(B, S, np.int32)
    spn[3], spn[5], spn[9] = S // 2, 0, 37
    for b in range(B):
        scan[b, spn[b]:] = 0.0
    mask = body_mask_golden() if V == 10475 else (rng.random(V) < 0.66)
    parents = np.where(SYN_PARENTS() < 0, -1, SYN_PARENTS())
    segm, par = segmentation_from_weights(prob['model']['weights'], faces, parents)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
    kw = dict(contact=dict(scene_v=t(scene, F32), contact_verts_ids=ids),
              scan=dict(scan=t(scan, F32), scan_point_num=t(spn, np.int32), body_mask=t(mask, bool)),
              selfpen=dict(faces_segm=segm, faces_parents=par, ign_part_pairs=['9,16'], selfpen=dict(SELFPEN)), velocity={})
    _SETUPS[key] = dict(prob=prob, faces=faces, kw=kw, scene=scene, ids=np.asarray(ids), scan=scan.astype(F32), spn=spn, mask=mask, plain={})
    return _SETUPS[key]


def case(lib, device, which):
    """-> (problem with the case's weights, keyword arguments, set-up)"""
    su = setup(lib, device, BIG[which])
    kw, w = {}, {}
    for p in parts_of(which):
        kw.update(su['kw'][p])
        w.update(WEIGHTS[p])
    if which == 'overflow':
        kw['selfpen'] = dict(SELFPEN, max_pairs=OVERFLOW_PAIRS)
    return dict(su['prob'], weights=dict(su['prob']['weights'], **w)), kw, su


def plain_engine_grads(lib, device, su, first, prob=None, key=''):
    """transl gradient, dverts and vertices of the engine WITHOUT the new arguments (once per set-up, flag and problem ``key``)"""
    if (first, key) not in su['plain']:
        eng = engine_for(prob or su['prob'], device, lib, first)
        eng.closure()
        su['plain'][first, key] = (eng.grads()['transl'].clone(), eng.ws['dverts'].clone(), eng.ws['verts'].clone())
    return su['plain'][first, key]


# ------------------------------------------------------------------------------------------------------------ 1 + 2: parity, liveness
def check_parity(lib, device, which, first):
    from lemo_amd.prox import ENGINE_PARAMS, LOSS_KEYS
    prob, kw, su = case(lib, device, which)
    fit = fitter_for(prob, device, lib, first, **kw)
    eng = engine_for(prob, device, lib, first, **kw)
    assert eng.terms is not None
    old = fit.closure()
    ld = eng.closure()
    for k in LOSS_KEYS:
        a, b = ld[k], float(old[k].detach())
        print(f'{which} first={first} {k}: engine {a:.9g}, fitter {b:.9g}')
        assert abs(a - b) <= 1e-5 * abs(b) + 1e-12, (k, a, b)
    # ---- the terms are live: for the fitter alone, and in the engine
    for p in parts_of(which):
        for k in TERM_KEYS[p]:
            assert float(old[k].detach()) > 0 and ld[k] > 0, k
    for k in set(sum(TERM_KEYS.values(), ())) - set(sum((TERM_KEYS[p] for p in parts_of(which)), ())):
        assert ld[k] == 0.0 and float(old[k].detach()) == 0.0, k
    g = eng.grads()
    assert not torch.equal(g['transl'], plain_engine_grads(lib, device, su, first)[0]), 'the term does not reach transl'
    T = eng._terms_t
    if 'selfpen' in parts_of(which):
        cnt = host(T['pair_count'])
        print(f'{which}: pairs per frame {cnt.tolist()} (max_pairs {eng.terms.max_pairs})')
        assert cnt.max() > 0
        assert (cnt.max() > eng.terms.max_pairs) == (which == 'overflow')
    if 'scan' in parts_of(which):
        c = host(T['counts'])
        live = (c[0] > 0) & (c[1] > 0)
        print(f'{which}: scan counts {c[0].tolist()}, visible {c[1].tolist()}, masked-visible {c[2].tolist()}')
        assert live.any() and (~live).any() and np.array_equal(c[0], su['spn'])
    # ---- gradients and one step
    for n, _ in ENGINE_PARAMS:
        ref = fit.pose_embedding.grad if n == 'pose_embedding' else getattr(fit.body_model, n).grad
        e = rel_err(g[n], ref)
        print(f'{which} first={first} grad {n}: rel_err {e:.2e}')
        assert e < 2e-4, (n, e)
    fit.optimizer.step()
    eng.step(1, use_graph=False)
    for n, _ in ENGINE_PARAMS:
        ref = fit.pose_embedding if n == 'pose_embedding' else getattr(fit.body_model, n)
        assert float((eng.P[n] - ref.detach()).abs().max()) < 2e-6, n
    assert eng.nonfinite_step() == 0


# ------------------------------------------------------------------------------------------------------------ 3: float64
def gmof(d, rho):
    return rho * rho * d / (d + rho * rho)


def terms_restated(verts, eng, prob, kw, su, parts, dtype):
    """The definitions (ProxTemporalFitter.loss_dict: prox.py, chamfer.contact_term, scan.scan_terms, selfpen_common.loss64) in torch
    at ``dtype`` with autograd, on the engine's vertices and decisions -> (values {key: float}, gradient [B, V, 3] float64)"""
    T, w = eng._terms_t, prob['weights']
    tt = lambda a: torch.from_numpy(np.asarray(a, F64)).to(dtype)
    v = tt(verts).requires_grad_(True)
    val, tot = {}, torch.zeros((), dtype=dtype)
    if 'contact' in parts:
        vw = v @ tt(prob['R']).T + tt(prob['t'])
        x = vw[:, torch.from_numpy(su['ids'].astype(np.int64))]
        nn = tt(su['scene'])[torch.from_numpy(host(T['cidx']).astype(np.int64))]
        s = torch.sqrt(((x - nn) ** 2).sum(-1) + 1e-4)
        val['contact_loss'] = w['contact_loss_weight'] * (s / (s + 1.0)).mean()
    if 'scan' in parts:
        c, vis, qm = host(T['counts']), host(T['vis']).astype(bool), host(T['qmask']).astype(bool)
        i_s, i_m, scan = host(T['s2m_idx']).astype(np.int64), host(T['m2s_idx']).astype(np.int64), tt(su['scan'])
        assert np.array_equal(qm, vis & su['mask'][None]) and np.array_equal(c[1], vis.sum(1)) and np.array_equal(c[2], qm.sum(1))
        s2m, m2s = [], []
        for b in range(B):
            if c[0][b] == 0 or c[1][b] == 0:
                continue
            n = int(c[0][b])
            assert (i_s[b, :n] >= 0).all() and vis[b][i_s[b, :n]].all()
            s2m.append(gmof(((scan[b, :n] - v[b][torch.from_numpy(i_s[b, :n])]) ** 2).sum(-1), w['rho_s2m']).mean())
            if c[2][b]:
                q = np.nonzero(qm[b])[0]
                assert (i_m[b, q] >= 0).all() and (i_m[b, q] < n).all()
                m2s.append(gmof(((v[b][torch.from_numpy(q)] - scan[b][torch.from_numpy(i_m[b, q])]) ** 2).sum(-1), w['rho_m2s']).mean())
        val['s2m_dist'], val['m2s_dist'] = w['s2m_weight'] * torch.stack(s2m).mean(), w['m2s_weight'] * torch.stack(m2s).mean()
    if 'velocity' in parts:
        mk = v[:, torch.from_numpy(np.asarray(prob['ids']['markers81'], np.int64))]
        vel = mk[1:] - mk[:-1]
        val['smooth_acc_loss'] = w['smooth_acc_weight'] * ((vel[1:] - vel[:-1]) ** 2).mean()
        val['smooth_vel_loss'] = w['smooth_vel_weight'] * (vel ** 2).mean()
    for x in val.values():
        tot = tot + x
    if tot.requires_grad:
        tot.backward()
    grad = v.grad.double().numpy() if v.grad is not None else np.zeros(verts.shape)
    val = {k: float(x) for k, x in val.items()}
    if 'selfpen' in parts:
        pairs, cnt = host(T['pairs']), host(T['pair_count'])
        lists = [pairs[b, :min(int(cnt[b]), pairs.shape[1])].astype(np.int64) for b in range(B)]
        cfg = kw['selfpen']
        L, g = loss64(np.asarray(verts, F64), su['faces'], lists, cfg['sigma'], cfg['penalize_outside'], dtype,
                      weights=np.full(B, w['coll_loss_weight']))
        val['self_penetration_loss'] = float(w['coll_loss_weight'] * L.sum())
        grad = grad + g
    return val, grad


def check_float64(lib, device, which):
    prob, kw, su = case(lib, device, which)
    parts = parts_of(which)
    # the S2 / S3 weights at 0: d(loss)/d(verts) of the window itself reaches 4e2 (the smoothness prior's 1e8), under which the
    # terms' share (1e-3 .. 1e1) could only be seen to two digits; the vertices do not depend on the weights
    quiet = {k: 0.0 for k in su['prob']['weights']}
    prob = dict(prob, weights=dict(prob['weights'], **quiet))
    eng = engine_for(prob, device, lib, False, **kw)
    ld = eng.closure()
    _, base, verts0 = plain_engine_grads(lib, device, su, False, dict(su['prob'], weights=quiet), 'quiet')
    assert torch.equal(eng.ws['verts'], verts0), 'the two engines do not see the same vertices'
    verts = host(eng.ws['verts']).astype(F64)
    got = host(eng.ws['dverts']).astype(F64) - host(base).astype(F64)
    v64, g64 = terms_restated(verts, eng, prob, kw, su, parts, torch.float64)
    v32, g32 = terms_restated(verts, eng, prob, kw, su, parts, torch.float32)
    for k, want in v64.items():
        bound = max(4 * abs(v32[k] - want) / want, 16 * EPS32)
        e = abs(ld[k] - want) / want
        print(f'{which} {k}: engine {ld[k]:.9g}, float64 {want:.9g}, rel {e:.2e} (bound {bound:.2e})')
        assert want > 0 and e <= bound, (k, e, bound)
    scale = np.abs(g64).max()
    bound = max(4 * np.abs(g32 - g64).max() / scale, 16 * EPS32) + 5 * EPS32 * float(eng.ws['dverts'].abs().max()) / scale
    e = np.abs(got - g64).max() / scale
    print(f'{which} gradient share: rel {e:.2e} (bound {bound:.2e}), max |share| {scale:.3g}, max |dverts| {float(eng.ws["dverts"].abs().max()):.3g}')
    assert scale > 0 and np.isfinite(got).all() and e <= bound, (e, bound)


# ------------------------------------------------------------------------------------------------------------ 4: reproducibility (GPU)
def _state(eng):
    st = eng.save_state()
    return [st[k] for k in sorted(st)] + [eng.ws['losses'].clone()]


def check_reproducible(lib, device):
    prob, kw, su = case(lib, device, 'all')
    runs = []
    for use_graph in (True, False, True):
        eng = engine_for(prob, device, lib, False, **kw)
        s = torch.cuda.Stream(device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):
            eng.step(3, use_graph=use_graph)
            s.synchronize()
            runs.append(_state(eng))
        assert eng.nonfinite_step() == 0 and eng.loss_dict()['self_penetration_loss'] > 0 and eng.loss_dict()['s2m_dist'] > 0
    for what, (a, b) in (('graph vs eager', (runs[0], runs[1])), ('engine A vs engine B', (runs[0], runs[2]))):
        for x, y in zip(a, b):
            assert torch.equal(x, y), what


# ------------------------------------------------------------------------------------------------------------ 5: untouched default
def check_default_untouched(lib, device, monkeypatch):
    prob, kw, su = case(lib, device, 'all')
    rec = _Recorder(lib.prox_set_terms)
    monkeypatch.setattr(lib, 'prox_set_terms', rec)
    plain = engine_for(su['prob'], device, lib, False)
    assert rec.calls == 0 and plain.terms is None
    zero = dict(su['prob'], weights=dict(su['prob']['weights'], **{k: 0.0 for p in SINGLE for k in WEIGHTS[p] if k.endswith('weight')}))
    quiet = engine_for(zero, device, lib, False, **kw)
    assert rec.calls == 0 and quiet.terms is None, 'arguments without a weight must not attach anything'
    live = engine_for(prob, device, lib, False, **kw)
    assert rec.calls == 1 and live.terms is not None
    monkeypatch.undo()
    for e in (plain, quiet):
        e.step(3, use_graph=False)
    for x, y in zip(_state(plain), _state(quiet)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 6: validation
def check_validation(lib, device):
    import ctypes as C
    from lemo_amd import _hip
    prob, kw, su = case(lib, device, 'contact')
    ids = su['ids']
    with pytest.raises(ValueError, match='contact_verts_ids must be unique'):
        engine_for(prob, device, lib, **dict(kw, contact_verts_ids=np.concatenate([ids, ids[:1]])))
    for make in (fitter_for, engine_for):
        sc = su['kw']['scan']
        with pytest.raises(ValueError, match='scan must be a float32'):
            make(su['prob'], device, lib, **dict(sc, scan=sc['scan'].double()))
        with pytest.raises(ValueError, match='scan must be a float32'):
            make(su['prob'], device, lib, **dict(sc, scan=sc['scan'].to('meta')))
        with pytest.raises(ValueError, match='faces_parents / ign_part_pairs need faces_segm'):
            make(su['prob'], device, lib, faces_parents=su['kw']['selfpen']['faces_parents'])
        with pytest.raises(ValueError, match='selfpen: unknown keys'):
            make(su['prob'], device, lib, selfpen=dict(height=1.0))
        with pytest.raises(ValueError, match='scan_point_num must lie in'):
            make(su['prob'], device, lib, **dict(sc, scan_point_num=sc['scan_point_num'] + S))
    # the C entry: NULL handle / struct, a NULL scratch pointer, a short workspace -> LEMO_ERR_ARG and nothing attached
    eng = engine_for(prob, device, lib, **kw)
    before = eng.closure()
    t = _hip.ProxTerms.from_buffer_copy(eng.terms)
    assert lib.prox_set_terms(None, C.byref(t)) == 10002 and lib.prox_set_terms(eng.handle, None) == 10002
    for field, value in (('contact_dist', None), ('contact_ws_bytes', max(eng.terms.contact_ws_bytes - 1, -1)), ('frame_acc', None),
                         ('contact_vid_host', None), ('contact_loss_weight', float('nan'))):
        bad = _hip.ProxTerms.from_buffer_copy(eng.terms)
        setattr(bad, field, value)
        if field == 'contact_ws_bytes' and eng.terms.contact_ws_bytes == 0:
            continue
        assert lib.prox_set_terms(eng.handle, C.byref(bad)) == 10002, field
    dup = np.ascontiguousarray(np.concatenate([ids[:-1], ids[:1]]), np.int32)          # the host copy is what the entry checks
    bad = _hip.ProxTerms.from_buffer_copy(eng.terms)
    bad.contact_vid_host = dup.ctypes.data
    assert lib.prox_set_terms(eng.handle, C.byref(bad)) == 10002, 'duplicate contact ids'
    faces = torch.from_numpy(np.ascontiguousarray(su['faces'], np.int32)).to(device)
    bad = _hip.ProxTerms.from_buffer_copy(eng.terms)
    bad.coll_loss_weight, bad.faces, bad.F, bad.sigma, bad.max_pairs = 0.01, faces.data_ptr(), int(faces.shape[0]), 0.5, 16
    assert lib.prox_set_terms(eng.handle, C.byref(bad)) == 10002, 'self-penetration without its scratch'
    after = eng.closure()
    assert before == after, 'a refused call changed the engine'


def check_layout():
    """the ctypes mirror of lemo_prox_terms has the C struct's size and offsets (tests/test_abi.py's method)"""
    import ctypes as C
    import subprocess
    import tempfile
    from lemo_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f for f, _ in _hip.ProxTerms._fields_]
    src = '#include <cstdio>\n#include <cstddef>\n#include "lemo_hip.h"\nint main(){\nprintf("%zu", sizeof(lemo_prox_terms));' + \
        ''.join(f'printf(" %zu", offsetof(lemo_prox_terms, {f}));' for f in names) + 'printf("\\n");return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, 'o.cpp'), 'w').write(src)
        subprocess.run(['g++', '-I', os.path.join(root, 'include'), os.path.join(td, 'o.cpp'), '-o', os.path.join(td, 'o')], check=True)
        want = [int(x) for x in subprocess.run([os.path.join(td, 'o')], check=True, capture_output=True, text=True).stdout.split()]
    assert [C.sizeof(_hip.ProxTerms)] + [getattr(_hip.ProxTerms, f).offset for f in names] == want


# ------------------------------------------------------------------------------------------------------------ 7: non-finite
def check_nonfinite(lib, device):
    prob, kw, su = case(lib, device, 'scan')
    sc = dict(kw, scan=kw['scan'].clone())
    eng = engine_for(prob, device, lib, True, **sc)
    eng.step(1, use_graph=False)
    assert eng.nonfinite_step() == 0
    sc['scan'][1, 7, 2] = float('nan')                            # a valid point of a live frame (the engine reads the caller's tensor)
    eng.step(1, use_graph=False)
    assert eng.nonfinite_step() == 2 and not np.isfinite(eng.loss_dict()['total_loss'])
    p = eng.P['transl'].clone()
    eng.step(2, use_graph=False)
    assert torch.equal(torch.nan_to_num(eng.P['transl'], nan=5.0), torch.nan_to_num(p, nan=5.0)) and int(eng.step_ctr.item()) == 4
