"""The cases of the dataset-builder tests, shared by the emulator suite (tests/test_dataset_emu.py) and the GPU suite
(tests/test_dataset_gpu.py).  Every figure is printed before it is asserted (``pytest -s`` shows them)."""
import functools

import numpy as np
import pytest
import torch

import dataset_common as DC
from lemo_amd import _hip, synthetic
from lemo_amd.body_model import SMPLX
from lemo_amd.dataset import ClipImageBuilder, divide_clips, load_stats, read_amass, save_stats

MODES = ('local_markers_4chan', 'local_markers')
# (T, M, N, chunk): T = 2 the shortest clip, 12 the filter clamped at both ends, 65 across a wave, 240 the 8 s default; every one
# with 67 and 81 markers, as one clip and as 5 clips in launches of 2 (per-clip offsets of images and partials)
SHAPES = [(T, M, N, ch) for T in (2, 12, 65, 120, 240) for M in (67, 81) for N, ch in ((1, 256), (5, 2))]


class _NoModel:
    use_pca = False

    class data:
        V = 1 << 30


def builder(lib, device, mode, M=67, chunk=256, models=None):
    return ClipImageBuilder(models or {'male': _NoModel()}, mode=mode, with_hand=M == 81, chunk=chunk, device=device, _lib=lib)


@functools.lru_cache(maxsize=None)
def fixture():
    return DC.load_fixture()


def t32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def ratio(got, ref, sens):
    """largest (|got - ref| - one fp32 rounding of ref) / sens: the gate asks for at most 4"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) - DC.EPS32 * np.abs(ref) - 1e-45
    return float(err.max() / sens) if sens > 0 else (0.0 if err.max() <= 0 else np.inf)


def fix_stats(fx, T, four):
    if four:
        return {k: fx[f'a{T}_stats_{k}'] for k in ('Xmean_local', 'Xstd_local', 'Xmean_global_xy', 'Xstd_global_xy', 'Xmean_global_r', 'Xstd_global_r')}
    return {k: fx[f's{T}_stats_{k}'] for k in ('Xmean', 'Xstd')}


# ---- 0. the yardstick against the reference's own output ---------------------------------------------------------------------
def check_restatement_is_the_reference():
    fx = fixture()
    for T in (30, 120):
        body, raw, rawg = fx[f'a{T}_body'], fx[f'a{T}_raw'], fx[f'a{T}_raw_g']
        full = np.concatenate([raw[:, None], rawg[..., None].repeat(raw.shape[-1], -1)], 1)
        for i in range(len(body)):
            img, _, lbl = DC.raw_4chan_from_body(body[i])
            assert np.abs(img - full[i]).max() < 1e-12
            assert np.array_equal(lbl[:-1], raw[i, :, -4:])
            m, p = DC.canonicalise(fx[f'm{T}_markers'][i], fx[f'm{T}_pelvis'][i], fx[f'm{T}_hips0'][i])
            mine = np.concatenate([p[:, None], m], 1)
            # numpy's and torch's fp32 products may round differently: three roundings of values below 4 m
            assert np.abs(mine - body[i]).max() <= 3 * DC.EPS32 * 4.0
            sm = DC.raw_smooth(fx[f'm{T}_markers'][i], fx[f'm{T}_pelvis'][i], fx[f'm{T}_hips0'][i])
            assert np.abs(sm - fx[f's{T}_raw'][i]).max() <= 6 * DC.EPS32 * 4.0
        st = DC.stats_4chan(full)
        assert all(np.array_equal(st[k], v) for k, v in fix_stats(fx, T, True).items())
        assert np.array_equal(DC.normalise_4chan(full, st)[:, 0].astype(np.float32), fx[f'a{T}_norm'])
        ss = DC.stats_smooth(fx[f's{T}_raw'])
        assert all(np.array_equal(ss[k], v) for k, v in fix_stats(fx, T, False).items())
        assert np.array_equal(DC.normalise_smooth(fx[f's{T}_raw'], ss)[:, :, :3], fx[f's{T}_norm3'])


# ---- 1. kernel on the reference's markers against the reference's images -----------------------------------------------------
def check_kernel_vs_fixture(lib, device, T):
    fx = fixture()
    mk, pv, hp = (t32(fx[f'm{T}_{k}'], device) for k in ('markers', 'pelvis', 'hips0'))
    b = builder(lib, device, MODES[0])
    vec = b._stats_vector(fix_stats(fx, T, True))
    img, piv, con = b.images_from_markers(mk, pv, hp, vec)
    img = img.cpu().numpy()
    sens = fx[f'a{T}_sens']
    assert np.array_equal(img[:, 0, -4:], fx[f'a{T}_raw'][:, :, -4:].transpose(0, 2, 1))                 # labels: exact
    assert np.array_equal(con.cpu().numpy()[:, :-1], fx[f'a{T}_raw'][:, :, -4:])
    r = [ratio(img[:, 0, :-4], fx[f'a{T}_norm'][:, :, :-4].transpose(0, 2, 1), sens[0])]
    for c in (1, 2, 3):
        assert np.array_equal(img[:, c], img[:, c, :1].repeat(img.shape[2], 1))                           # one value per frame
        r.append(ratio(img[:, c, 0], fx[f'a{T}_norm_g'][:, c - 1], sens[c]))
    print(f'4chan T={T}: error / sens per channel', np.round(r, 3))
    assert max(r) <= 4.0, r
    b = builder(lib, device, MODES[1])
    img, _, _ = b.images_from_markers(mk, pv, hp, b._stats_vector(fix_stats(fx, T, False)))
    img = img.cpu().numpy()[:, 0].transpose(0, 2, 1)
    sens = fx[f's{T}_sens']
    r = [ratio(img[:, :, :3], fx[f's{T}_norm3'], sens[0]), ratio(img[:, :, 3:], fx[f's{T}_raw'][:, :, 3:], sens[1])]
    print(f'smooth T={T}: error / sens (pelvis rows, marker rows)', np.round(r, 3))
    assert max(r) <= 4.0, r
    return r


# ---- 2. / 3. kernel against the restatement across shapes; statistics ---------------------------------------------------------
def restate(mode, mk, pv, hp):
    """(raw [N, C, F, d] float64, rot_0_pivot, labels) of the restatement"""
    if mode == MODES[0]:
        out = [DC.raw_4chan(mk[i], pv[i], hp[i]) for i in range(len(mk))]
        return np.stack([o[0] for o in out]), np.array([o[1][0] for o in out]), np.stack([o[2] for o in out])
    return np.stack([DC.raw_smooth(mk[i], pv[i], hp[i]) for i in range(len(mk))])[:, None].astype(np.float64), None, None


def normalise(mode, raw, vec):
    d = raw.shape[-1]
    out = raw.copy()
    if mode == MODES[0]:
        out[:, 0] = (raw[:, 0] - vec[:d]) / vec[d:2 * d]
        out[:, 1:3] = (raw[:, 1:3] - vec[2 * d]) / vec[2 * d + 1]
        out[:, 3] = (raw[:, 3] - vec[2 * d + 2]) / vec[2 * d + 3]
    else:
        out[..., :3] = (raw[..., :3] - vec[:3]) / vec[d:d + 3]
    return out


def channels(mode, img):
    """the groups a sens figure is taken over: [N, C, F, d] -> list of arrays"""
    if mode == MODES[0]:
        return [img[:, 0, :, :-4], img[:, 1], img[:, 2], img[:, 3]]
    return [img[:, 0, :, :3], img[:, 0, :, 3:]]


def check_shape(lib, device, mode, T, M, N, chunk):
    four = mode == MODES[0]
    mk, pv, hp = DC.synthetic_markers(7 * T + M + N, N, T, M)
    for i in range(N):                                          # the inputs keep clear of the label thresholds
        m, _ = DC.canonicalise(mk[i], pv[i], hp[i])
        speed, height, thr = DC.foot_margins(m)
        assert np.abs(speed - 0.22).min() > 1e-5 and np.abs(height - thr).min() > 1e-5
    raw, piv, lbl = restate(mode, mk, pv, hp)
    b = builder(lib, device, mode, M, chunk)
    dev = [t32(a, device) for a in (mk, pv, hp)]
    got_raw, got_piv, got_con = b.images_from_markers(*dev)
    got_raw = got_raw.cpu().numpy().transpose(0, 1, 3, 2)
    if four:
        assert np.array_equal(got_con.cpu().numpy(), lbl) and np.array_equal(got_raw[:, 0, :, -4:], lbl[:, :-1])
        assert np.abs(got_piv.cpu().numpy() - piv).max() < 1e-9, np.abs(got_piv.cpu().numpy() - piv).max()
    raw_of = lambda *a: tuple(channels(mode, restate(mode, *a)[0]))
    sens = DC.sens_of(raw_of, (mk, pv, hp))
    r = [ratio(g, w, s) for g, w, s in zip(channels(mode, got_raw), channels(mode, raw), sens)]
    print(f'{mode} T={T} M={M} N={N}: raw error / sens', np.round(r, 3))
    assert max(r) <= 4.0, r
    # ---- statistics: numpy float64 on the restatement's images, 10 n 2^-53 with n the number of terms summed
    vec = b.stats_from_markers(*dev).cpu().numpy()
    d, F = raw.shape[-1], raw.shape[2]
    u = 10.0 * 2.0 ** -53
    want = DC.stats_f64(raw if four else raw[:, 0], four)
    nb = d - 4 if four else d
    # absolute scale of a sum of n entries: n times the size of what an entry is computed FROM, not of the entry -- a rotated
    # coordinate is c x + s y with |x|, |y| up to S, and the kernel's and numpy's float64 evaluations of it differ by a few
    # 2^-53 S however small the result (with n = 1, one clip of two frames, that is all the difference there is)
    S = np.abs(raw[:, 0, :, :nb]).max()
    tol_mean = u * N * F * S
    assert np.all(np.abs(vec[:nb] - want[:nb]) <= tol_mean + 1e-300), np.abs(vec[:nb] - want[:nb]).max()
    assert np.array_equal(vec[nb:d], want[nb:d]) and np.array_equal(vec[d + nb:2 * d], want[d + nb:2 * d])
    # standard deviations: the summation error, relative to the std, plus the same entry-level term as for the means (every
    # entry carries a few 2^-53 of its operands' size, which a small std -- the heading change of a short, filtered clip is
    # 1e-6 rad -- does not shrink); a single entry (one clip of two frames has ONE heading change) must give exactly zero
    def rel(a, w, scale=0.0):
        return abs(a - w) / (abs(w) + scale) if w != 0 else (0.0 if a == 0 else np.inf)
    assert rel(vec[d + 3], want[d + 3], S) <= u * N * F * d and np.all(vec[d + 3:d + nb] == vec[d + 3])
    if four:
        assert vec[d] == vec[d + 3]
        assert abs(vec[2 * d] - want[2 * d]) <= u * 2 * N * F * np.sqrt((raw[:, 1:3, :, 0] ** 2).sum(1)).max()      # |(dx, dz)|: the rotation keeps it
        assert rel(vec[2 * d + 1], want[2 * d + 1], np.sqrt((raw[:, 1:3, :, 0] ** 2).sum(1)).max()) <= u * 2 * N * F
        assert abs(vec[2 * d + 2] - want[2 * d + 2]) <= u * N * F * 1.0            # computed from unit quaternions: operands of size 1
        assert rel(vec[2 * d + 3], want[2 * d + 3], 1.0) <= u * N * F
    else:
        assert rel(vec[d], want[d], S) <= u * N * F * 3 and vec[d + 1] == vec[d] and vec[d + 2] == vec[d]
    # normalising needs every std above zero: not so for channel 3 of a single two-frame clip (F = 1, N = 1), where the loader divides by zero too
    if all(want[k] > 0 for k in ((d, 2 * d + 1, 2 * d + 3) if four else (d, d + 3))):
        # ---- normalised image against the restatement normalised with ITS statistics
        ref = normalise(mode, raw, want)
        got, _, _ = b.images_from_markers(*dev, torch.from_numpy(vec))
        got = got.cpu().numpy().transpose(0, 1, 3, 2)

        def norm_of(*a):
            rr = restate(mode, *a)[0]
            return tuple(channels(mode, normalise(mode, rr, DC.stats_f64(rr if four else rr[:, 0], four))))
        sens = DC.sens_of(norm_of, (mk, pv, hp))
        r = [ratio(g, w, s) for g, w, s in zip(channels(mode, got), channels(mode, ref), sens)]
        print(f'{mode} T={T} M={M} N={N}: normalised error / sens', np.round(r, 3))
        assert max(r) <= 4.0, r
    if N > 1:                                                   # chunking and repetition change no bit
        for ch in (1, 2, 5):
            bb = builder(lib, device, mode, M, ch)
            assert np.array_equal(bb.stats_from_markers(*dev).cpu().numpy(), vec)
            assert torch.equal(bb.images_from_markers(*dev)[0].cpu().transpose(2, 3), torch.from_numpy(got_raw).float())
        assert np.array_equal(b.stats_from_markers(*dev).cpu().numpy(), vec)


# ---- 4. layout ---------------------------------------------------------------------------------------------------------------
def check_layout(lib, device, T=65):
    from lemo_amd.markers import get_local_markers_4chan
    mk, pv, hp = DC.synthetic_markers(5, 2, T)
    b = builder(lib, device, MODES[0])
    dev = [t32(a, device) for a in (mk, pv, hp)]
    img, piv, con = b.images_from_markers(*dev)
    api, _, _ = b.images_from_markers(*dev, api_layout=True)
    assert torch.equal(api.permute(0, 1, 3, 2), img)
    for i in range(2):
        m, p = DC.canonicalise(mk[i], pv[i], hp[i])
        body = t32(np.concatenate([p[:, None], m], 1), device)
        old, old_piv = get_local_markers_4chan(body, con[i], _lib=lib)
        a, w = img[i].cpu().double().numpy(), old.permute(0, 2, 1).cpu().double().numpy()
        # one fp32 ulp of the value, plus half an ulp of the largest operand of its channel: every entry is a sum of products of
        # such operands (rotation by the heading), and the two kernels see the heading through floor shifts rounded in fp32
        # (here, like the loader) and in float64 (there, like utils.get_local_markers_4chan on float64 input)
        S = np.abs(w).max(axis=(1, 2), keepdims=True)
        assert np.all(np.abs(a - w) <= 2.0 ** -23 * np.abs(w) + 2.0 ** -24 * S), (np.abs(a - w) / (2.0 ** -23 * np.abs(w) + 2.0 ** -24 * S)).max()
        assert abs(float(old_piv[0]) - float(piv[i])) < 2.0 ** -23


# ---- 5. round trip through lemo_decode_clip ----------------------------------------------------------------------------------
def decode(lib, device, img, vec, piv, M):
    """img [4, d, F] float32 normalised -> markers [F, M, 3]"""
    d, F = img.shape[1], img.shape[2]
    rec, traj = img[0].contiguous(), img[1:, 0].contiguous()
    lbl = torch.empty(F, 4, dtype=torch.float32, device=device)
    out = torch.empty(F, M, 3, dtype=torch.float32, device=device)
    lib.check(lib.decode_clip(_hip.ptr(rec), _hip.ptr(traj), _hip.ptr(vec), _hip.ptr(piv), None, F, M + 1, _hip.ptr(lbl), _hip.ptr(out),
                              lib.stream(device)), 'decode_clip')
    return out.cpu().numpy().astype(np.float64), lbl.cpu().numpy()


def check_round_trip(lib, device, T=65, N=3):
    mk, pv, hp = DC.synthetic_markers(21, N, T)
    b = builder(lib, device, MODES[0])
    dev = [t32(a, device) for a in (mk, pv, hp)]
    vec = b.stats_from_markers(*dev)
    img, piv, con = b.images_from_markers(*dev, vec)
    raw, rpiv, lbl = restate(MODES[0], mk, pv, hp)
    ref_img = torch.from_numpy(normalise(MODES[0], raw, vec.cpu().numpy()).transpose(0, 1, 3, 2).astype(np.float32)).to(device)
    worst = 0.0
    for i in range(N):
        m, p = DC.canonicalise(mk[i], pv[i], hp[i])
        want = m[:-1].astype(np.float64)
        want[:, :, 2] -= float(min(m[:, :, 2].min(), p[:, 2].min()))
        got, got_lbl = decode(lib, device, img[i], vec, piv[i:i + 1].contiguous(), 67)
        own, _ = decode(lib, device, ref_img[i].contiguous(), vec, torch.tensor([rpiv[i]], dtype=torch.float64, device=device), 67)
        e_got, e_own = np.abs(got - want).max(), np.abs(own - want).max()
        print(f'round trip clip {i}: builder {e_got:.3e}  restatement {e_own:.3e}')
        assert e_got <= 4.0 * e_own and e_own < 1e-4
        assert np.array_equal(got_lbl, lbl[i, :-1])
        worst = max(worst, e_got / e_own)
    return worst


# ---- 6. end to end from parameters -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def models(lib):
    return {g: SMPLX(synthetic.make_synthetic_smplx(seed=s), gender=g, use_pca=False, flat_hand_mean=True, _lib=lib)
            for g, s in (('male', 0), ('female', 1))}


def fixture_clips(T):
    fx = fixture()
    return [dict(poses=fx[f'c{T}_poses'][i].astype(np.float64), trans=fx[f'c{T}_trans'][i].astype(np.float64), betas=fx[f'c{T}_betas'][i],
                 gender=str(fx[f'c{T}_gender'][i]), mocap_framerate=120) for i in range(len(fx[f'c{T}_poses']))]


def check_end_to_end(lib, device, tmp_path, T=30):
    fx = fixture()
    clips = fixture_clips(T)
    b = builder(lib, device, MODES[0], chunk=3, models=models(lib))
    mk, pv, hp = b._markers(clips, T)
    ref = fx[f'm{T}_markers']
    # the module's vertex gate (smoke(): vertices to 1e-4 relative) on everything the kernels are fed: markers, joint 0 of every
    # frame and joints 1-2 of frame 0 (these come from the pose stage's joints plus the translation, not from the vertex path)
    delta = 0.0
    for name, got in (('markers', mk), ('pelvis', pv), ('hips0', hp)):
        ref = fx[f'm{T}_{name}']
        assert tuple(got.shape) == ref.shape
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f'{name} against the reference, relative', err / np.abs(ref).max())
        assert err / np.abs(ref).max() < 1e-4
        delta = max(delta, err)
    img, info = b.build(clips)
    assert img.device == mk.device and img.shape == (len(clips), 4, 208, T - 1) and info['rot_0_pivot'].shape == (len(clips),)
    mkn, pvn, hpn = (a.cpu().numpy() for a in (mk, pv, hp))
    raw, _, lbl = restate(MODES[0], mkn, pvn, hpn)
    want = normalise(MODES[0], raw, DC.stats_f64(raw, True))
    got = img.cpu().numpy().transpose(0, 1, 3, 2)
    assert np.array_equal(info['contact'].cpu().numpy(), lbl)
    r = [ratio(g, w, s) for g, w, s in zip(channels(MODES[0], got), channels(MODES[0], want), fx[f'a{T}_sens'])]
    print('end to end: error / sens per channel against the restatement on the product\'s markers', np.round(r, 3))
    assert max(r) <= 4.0, r
    # the reference's image itself.  `sens` is what moving every input by ONE ulp does to the reference's image; the product's
    # inputs are `delta` away from the reference's, i.e. delta / ulp such steps (ulp: the median spacing of the reference's
    # marker coordinates, what the recorded perturbations typically moved a value by), and the chain is smooth in its inputs
    # away from the label thresholds (which the fixture keeps clear of by 1e-4, far more than delta): so the image may be
    # 4 sens (the gate) times that many steps away, plus the fp32 rounding of the stored value
    steps = max(1.0, delta / float(np.median(np.spacing(np.abs(fx[f'm{T}_markers'])))))
    refs = [fx[f'a{T}_norm'][:, :, :-4]] + [fx[f'a{T}_norm_g'][:, c] for c in range(3)]
    gots = [got[:, 0, :, :-4]] + [got[:, c, :, 0] for c in (1, 2, 3)]
    r = [ratio(g, w, s * steps) for g, w, s in zip(gots, refs, fx[f'a{T}_sens'])]
    print(f'end to end: inputs {delta:.2e} = {steps:.1f} ulp from the reference\'s; image error / (sens x steps) per channel', np.round(r, 3))
    assert max(r) <= 4.0, r
    assert np.array_equal(got[:, 0, :, -4:], fx[f'a{T}_raw'][:, :, -4:])                        # the reference's labels, exactly
    # test split: statistics saved and loaded
    path = str(tmp_path / 'stats.npz')
    save_stats(path, info['stats'])
    loaded = load_stats(path)
    assert set(loaded) == set(fix_stats(fx, T, True))
    again, _ = b.build(clips, stats=loaded)
    assert torch.equal(again, img)
    rawimg, _ = b.build(clips, normalize=False)
    assert np.array_equal(rawimg.cpu().numpy()[:, 0, -4:], got[:, 0, :, -4:].transpose(0, 2, 1))
    sm = builder(lib, device, MODES[1], models=models(lib))
    simg, sinfo = sm.build(clips)
    assert simg.shape == (len(clips), 1, 204, T) and sinfo['rot_0_pivot'] is None and set(sinfo['stats']) == {'Xmean', 'Xstd'}
    return img


# ---- 7. clip division and argument validation --------------------------------------------------------------------------------
def check_divide_clips(tmp_path):
    fx = fixture()
    seqs = DC.amass_sequences()
    got = divide_clips(seqs, clip_seconds=1)
    recs = []
    for c in got:
        src = [i for i, s in enumerate(seqs) if np.array_equal(s['betas'][:10], c['betas'])][0]
        start = int(np.nonzero((seqs[src]['poses'] == c['poses'][0]).all(1))[0][0])
        recs.append([src, start, len(c['poses']), c['mocap_framerate'], float(c['poses'].sum()), float(c['trans'].sum())])
        assert c['gender'] == str(seqs[src]['gender']) and c['betas'].shape == (10,)
    assert np.array_equal(np.asarray(sorted(recs), np.float64), fx['div_clips'])
    for i, s in enumerate(seqs):
        (tmp_path / 'DS' / f'subj{i}').mkdir(parents=True)
        np.savez(str(tmp_path / 'DS' / f'subj{i}' / f'seq{i}_poses.npz'), **s)
    np.savez(str(tmp_path / 'DS' / 'subj0' / 'shape.npz'), betas=np.zeros(16))          # not a *_poses.npz file
    read = read_amass(str(tmp_path), ['DS'], clip_seconds=1)
    key = lambda c: float(c['poses'].sum())
    assert [key(c) for c in sorted(read, key=key)] == [key(c) for c in sorted(got, key=key)]


def check_validation(lib, device, monkeypatch):
    launched = []
    for name in ('smplx_pose_fwd', 'clip_repr_stats', 'clip_repr_write', 'lbs_verts_fwd_active'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    good = DC.synthetic_clips(1, 2, 12)
    b = builder(lib, device, MODES[0])
    mod = lambda i, **kw: [dict(c, **kw) if j == i else c for j, c in enumerate(good)]
    cases = [mod(0, poses=good[0]['poses'][:, :150]),                                   # pose width
             mod(1, gender='neutral'),                                                  # no model for it
             mod(1, poses=good[1]['poses'][:8], trans=good[1]['trans'][:8]),            # unequal T
             [dict(c, poses=c['poses'][:1], trans=c['trans'][:1]) for c in good],       # T = 1
             [dict(c, poses=np.zeros((257, 156)), trans=np.zeros((257, 3))) for c in good],      # T = 257
             []]
    for clips in cases:
        for call in (b.build, b.compute_stats):
            with pytest.raises(ValueError):
                call(clips)
    with pytest.raises(ValueError):
        b.build(good, stats=dict(Xmean=np.zeros(204), Xstd=np.ones(204)))               # the other mode's statistics
    with pytest.raises(ValueError):
        ClipImageBuilder({'male': _NoModel()}, mode='global_markers', _lib=lib)
    assert launched == []
    # the native layer refuses the same shapes on its own
    d = _hip.ClipReprDesc(markers=1, pelvis=1, hips0=1, n_clips=1, T=257, M=67, mode=0, fps=30.0, image=1, stats_part=1)
    monkeypatch.undo()
    for T, M in ((257, 67), (1, 67), (30, 60), (30, 84)):
        d.T, d.M = T, M
        assert lib.clip_repr_write(d, None) == 10001 and lib.clip_repr_stats(d, None) == 10001
