"""The cases of the ``global_markers`` dataset-builder tests (lemo_amd.dataset.SmoothClipImageBuilder, mode LEMO_CLIP_GLOBAL of
csrc/dataset_kernels.hip), shared by the emulator suite (tests/test_dataset_global_emu.py) and the GPU suite
(tests/test_dataset_global_gpu.py).  Every figure is printed before it is asserted (``pytest -s`` shows them).

The yardsticks are the reference's own output (tests/golden/dataset_repr_global*.npz, written by make_dataset_global.py from
loader/train_loader_smooth.py in its default mode) and, at the shapes the fixture does not cover, a numpy restatement that
``check_restatement_is_the_reference`` first holds to that fixture.  The gate of every image comparison is the one of
tests/dataset_checks.py: 4 x ``sens``, the change of the yardstick's image under one-ulp moves of its float32 inputs.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import dataset_checks as K
import dataset_common as DC
from lemo_amd import _hip
from lemo_amd.dataset import ClipImageBuilder, SmoothClipImageBuilder, load_stats, save_stats

MS = (67, 81)
# (T, M, N, chunk): T = 2 the shortest clip, 12 under one wave, 65 across a wave, 120 the prior's clip, 240 all but a workgroup;
# both marker sets; one clip, and 5 clips in launches of 2 (per-clip offsets of images and partials, a last launch of 1)
SHAPES = [(T, M, N, ch) for T in (2, 12, 65, 120, 240) for M in MS for N, ch in ((1, 256), (5, 2))]
U = 10.0 * 2.0 ** -53                                          # the statistics bound of tests/dataset_checks.py, per term summed
GUARD, SENTINEL = 1024, -12345.0


@functools.lru_cache(maxsize=None)
def fixture():
    out = dict(K.fixture())
    for name in ('dataset_repr_global.npz', 'dataset_repr_global_norm.npz'):                 # two files: 1 MiB each at most
        with np.load(os.path.join(DC.GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def ref_markers(T, M):
    """the reference's float32 world-frame markers, joint 0 and first-frame joints 1-2 of the fixture's clips"""
    fx = fixture()
    mk = fx[f'm{T}_markers']
    if M == 81:
        mk = np.concatenate([mk, fx[f'g{T}_m81_extra']], 2)
    return mk, fx[f'm{T}_pelvis'], fx[f'm{T}_hips0']


def ref_stats(T, M):
    fx = fixture()
    return dict(Xmean=fx[f'g{T}_stats{M}_Xmean'], Xstd=fx[f'g{T}_stats{M}_Xstd'])


def builder(lib, device, M=67, chunk=256, models=None):
    return SmoothClipImageBuilder(models or {'male': K._NoModel()}, with_hand=M == 81, chunk=chunk, device=device, _lib=lib)


# ---- the restatement (train_loader_smooth.py:130-143, 164-167, 184-194) ------------------------------------------------------
def raw_global(markers, pelvis, hips0):
    """one clip -> image [T, 3 M] float32"""
    m, _ = DC.canonicalise(markers, pelvis, hips0, smooth=True)
    return m.reshape(len(m), -1)


def stats_global(imgs):
    """on [N, T, d]; float32 input gives the loader's float32 reductions, float64 input the yardstick of the native pass"""
    return dict(Xmean=imgs.mean(axis=1).mean(axis=0)[np.newaxis, np.newaxis, :], Xstd=np.ones(imgs.shape[-1]) * imgs.std())


def normalise_global(imgs, s):
    return (imgs - s['Xmean']) / s['Xstd']


def restate(mk, pv, hp):
    return np.stack([raw_global(mk[i], pv[i], hp[i]) for i in range(len(mk))])


def restate_norm(mk, pv, hp, stats=None):
    """float64 normalisation of the float32 image, with the float64 statistics of that image unless given"""
    raw = restate(mk, pv, hp).astype(np.float64)
    s = stats_global(raw) if stats is None else stats
    return (raw - np.asarray(s['Xmean'], np.float64)) / np.asarray(s['Xstd'], np.float64)


def frames_major(img):
    """[N, 1, d, T] device tensor -> [N, T, d] numpy"""
    return img.cpu().numpy()[:, 0].transpose(0, 2, 1)


# ---- 0. the yardstick against the reference's own output ---------------------------------------------------------------------
def check_restatement_is_the_reference():
    fx = fixture()
    for T in (30, 120):
        for M in MS:
            mk, pv, hp = ref_markers(T, M)
            raw, norm = fx[f'g{T}_raw{M}'], fx[f'g{T}_norm{M}']
            assert raw.dtype == np.float32 and raw.shape == (len(mk), T, 3 * M) and np.abs(raw).max() < 4.0
            mine = restate(mk, pv, hp)
            # numpy's and torch's fp32 products may round differently: three roundings of values below 4 m
            assert mine.dtype == np.float32 and np.abs(mine - raw).max() <= 3 * DC.EPS32 * 4.0
            st = stats_global(raw)
            assert all(np.array_equal(st[k], v) and st[k].dtype == v.dtype and st[k].shape == v.shape for k, v in ref_stats(T, M).items())
            assert np.array_equal(normalise_global(raw, st).astype(np.float32), norm)


# ---- 1. kernel on the reference's markers against the reference's images -----------------------------------------------------
def check_kernel_vs_fixture(lib, device, T, M):
    fx = fixture()
    b = builder(lib, device, M)
    dev = [K.t32(a, device) for a in ref_markers(T, M)]
    img, piv, con = b.images_from_markers(*dev, b._stats_vector(ref_stats(T, M)))
    assert piv is None and con is None and tuple(img.shape) == (len(dev[0]), 1, 3 * M, T)
    r = K.ratio(frames_major(img), fx[f'g{T}_norm{M}'], fx[f'g{T}_sens'][MS.index(M)])
    print(f'global_markers T={T} M={M}: error / sens against the reference\'s normalised image {r:.3f}')
    assert r <= 4.0, r
    return r


# ---- 2. end to end from AMASS parameters -------------------------------------------------------------------------------------
def check_end_to_end(lib, device, tmp_path, M, T=30):
    fx = fixture()
    clips = K.fixture_clips(T)
    assert len({c['gender'] for c in clips[:3]}) == 2            # chunk 3: both genders inside the first chunk
    b = builder(lib, device, M, chunk=3, models=K.models(lib))
    mk, pv, hp = b._markers(clips, T)
    delta = 0.0
    for name, got, ref in zip(('markers', 'pelvis', 'hips0'), (mk, pv, hp), ref_markers(T, M)):
        assert tuple(got.shape) == ref.shape
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f'{name} against the reference, relative', err / np.abs(ref).max())
        assert err / np.abs(ref).max() < 1e-4                   # the module's vertex gate
        delta = max(delta, err)
    img, info = b.build(clips)
    d = 3 * M
    assert img.device == mk.device and tuple(img.shape) == (len(clips), 1, d, T) and img.dtype == torch.float32
    assert info['rot_0_pivot'] is None and info['contact'] is None
    st = info['stats']
    assert set(st) == {'Xmean', 'Xstd'} and st['Xmean'].shape == (1, 1, d) and st['Xmean'].dtype == np.float32
    assert st['Xstd'].shape == (d,) and st['Xstd'].dtype == np.float64
    got = frames_major(img)
    mkn, pvn, hpn = (a.cpu().numpy() for a in (mk, pv, hp))
    sens = fx[f'g{T}_sens'][MS.index(M)]
    r = K.ratio(got, restate_norm(mkn, pvn, hpn, st), sens)
    print(f'end to end M={M}: error / sens against the restatement on the product\'s markers, normalised with the statistics handed out {r:.3f}')
    assert r <= 4.0, r
    # the reference's image itself: the product's inputs are `delta` away from the reference's, i.e. delta / ulp one-ulp steps
    # (tests/dataset_checks.py::check_end_to_end), and the chain is smooth in its inputs: 4 sens times that many steps
    steps = max(1.0, delta / float(np.median(np.spacing(np.abs(ref_markers(T, M)[0])))))
    r = K.ratio(got, fx[f'g{T}_norm{M}'], sens * steps)
    print(f'end to end M={M}: inputs {delta:.2e} = {steps:.1f} ulp from the reference\'s; image error / (sens x steps) {r:.3f}')
    assert r <= 4.0, r
    # test split: statistics saved, loaded, handed back; and computed on their own
    path = str(tmp_path / f'stats{M}.npz')
    save_stats(path, st)
    loaded = load_stats(path)
    assert all(np.array_equal(loaded[k], st[k]) and loaded[k].dtype == st[k].dtype for k in st)
    again, _ = b.build(clips, stats=loaded)
    assert torch.equal(again, img)
    own = b.compute_stats(clips)
    assert all(np.array_equal(own[k], st[k]) and own[k].dtype == st[k].dtype for k in st)
    api, _ = b.build(clips, api_layout=True)
    assert tuple(api.shape) == (len(clips), T, d) and torch.equal(api.permute(0, 2, 1), img[:, 0])
    rawimg, rinfo = b.build(clips, normalize=False)
    assert rinfo['stats'] is None and tuple(rawimg.shape) == tuple(img.shape)
    assert np.all(frames_major(rawimg)[:, 0, :3] == 0.0)          # marker 0 of frame 0 is the origin
    return img, info


# ---- 3. statistics -----------------------------------------------------------------------------------------------------------
def check_statistics(lib, device, T, M):
    """The native pass sums what its own fp32 canonicalisation gives, and that is not the reference's raw image bit for bit
    (torch's matmul and the kernel's fma round 12-14 % of the entries one ulp apart).  To hold the SUMS to float64 numpy of the
    reference's raw images, these are fed in as markers that are canonical already: marker 0 of frame 0 is the origin and hips
    along x make R0 the identity, so the kernel's image is the reference's raw image exactly (asserted) and the statistics
    pass adds exactly the reference's numbers."""
    fx = fixture()
    raw = fx[f'g{T}_raw{M}']
    N, d = len(raw), 3 * M
    assert np.all(raw[:, 0, :3] == 0.0)
    mk = K.t32(raw.reshape(N, T, M, 3), device)
    pv = torch.zeros(N, T, 3, device=device)
    hp = K.t32(np.tile(np.array([[0, 0, 0], [1, 0, 0]], np.float32), (N, 1, 1)), device)
    b = builder(lib, device, M)
    img, _, _ = b.images_from_markers(mk, pv, hp)
    assert np.array_equal(frames_major(img).view(np.int32), raw.view(np.int32))
    vec = b.stats_from_markers(mk, pv, hp).cpu().numpy()
    assert vec.shape == (2 * d + 4,)
    want = stats_global(raw.astype(np.float64))
    S, n = float(np.abs(raw).max()), N * T
    e_mean = float(np.abs(vec[:d] - want['Xmean'].reshape(-1)).max())
    e_std = abs(vec[d] - want['Xstd'][0]) / (want['Xstd'][0] + S)
    print(f'statistics T={T} M={M}: mean error {e_mean:.2e} (bound {U * n * S:.2e}), std error relative to std + operand size {e_std:.2e} (bound {U * n * d:.2e})')
    assert e_mean <= U * n * S and e_std <= U * n * d
    assert np.all(vec[d:2 * d] == vec[d]) and vec[2 * d] == vec[d] and vec[2 * d + 1] == vec[d] and vec[2 * d + 2] == 0 and vec[2 * d + 3] == 0
    # the reference's own saved statistics: float32 reductions, `gap` away from float64 ones of the same array (measured by
    # the generator on the reference alone)
    gap = fx[f'g{T}_stats_f32_gap'][MS.index(M)]
    saved = ref_stats(T, M)
    e_mean = float(np.abs(vec[:d] - saved['Xmean'].reshape(-1).astype(np.float64)).max())
    e_std = abs(vec[d] - saved['Xstd'][0])
    print(f'statistics T={T} M={M}: against the saved ones: mean {e_mean:.2e} (gap {gap[0]:.2e}), std {e_std:.2e} (gap {gap[1]:.2e})')
    assert e_mean <= gap[0] + U * n * S and e_std <= gap[1] + U * n * d * (want['Xstd'][0] + S)
    # from the reference's world-frame markers: the same bound against float64 numpy of the image the kernel itself writes
    dev = [K.t32(a, device) for a in ref_markers(T, M)]
    own = frames_major(b.images_from_markers(*dev)[0]).astype(np.float64)
    vec = b.stats_from_markers(*dev).cpu().numpy()
    w = stats_global(own)
    S = float(np.abs(own).max())
    assert np.abs(vec[:d] - w['Xmean'].reshape(-1)).max() <= U * n * S and abs(vec[d] - w['Xstd'][0]) / (w['Xstd'][0] + S) <= U * n * d
    # chunking and repetition change no bit
    for ch in (1, 2, 5):
        assert np.array_equal(builder(lib, device, M, ch).stats_from_markers(*dev).cpu().numpy(), vec)
    assert np.array_equal(b.stats_from_markers(*dev).cpu().numpy(), vec)
    dct = b._stats_dict(torch.from_numpy(vec))
    assert dct['Xmean'].dtype == np.float32 and dct['Xmean'].shape == (1, 1, d) and dct['Xstd'].dtype == np.float64 and dct['Xstd'].shape == (d,)
    assert np.all(dct['Xstd'] == dct['Xstd'][0])


# ---- 4. indexing sweep -------------------------------------------------------------------------------------------------------
def guarded_write(b, dev, vec, api):
    """the write pass into the middle of a buffer of sentinels -> (image [N, d, T] or [N, T, d], the whole buffer)"""
    mk, pv, hp = dev
    N, T, d = mk.shape[0], mk.shape[1], b.d
    buf = torch.full((2 * GUARD + N * d * T,), SENTINEL, dtype=torch.float32, device=b.device)
    s = b.lib.stream(b.device)
    for lo in range(0, N, b.chunk):
        hi = min(N, lo + b.chunk)
        desc = b._desc(mk, pv, hp, lo, hi, stats=_hip.ptr(vec), image=_hip.ptr(buf[GUARD + lo * d * T:]), api_layout=int(api))
        b.lib.check(b.lib.clip_repr_write(C.byref(desc), s), 'clip_repr_write')
    return buf[GUARD:GUARD + N * d * T].view((N, T, d) if api else (N, d, T)), buf


def check_shape(lib, device, T, M, N, chunk):
    mk, pv, hp = DC.synthetic_markers(11 * T + M + N, N, T, M)
    d = 3 * M
    b = builder(lib, device, M, chunk)
    dev = [K.t32(a, device) for a in (mk, pv, hp)]
    raw = restate(mk, pv, hp)
    got_raw = frames_major(b.images_from_markers(*dev)[0])
    sens = DC.sens_of(restate, (mk, pv, hp))[0]
    r = K.ratio(got_raw, raw, sens)
    print(f'global_markers T={T} M={M} N={N}: raw error / sens {r:.3f}')
    assert r <= 4.0, r
    # statistics against float64 numpy of the restatement's image
    vec_t = b.stats_from_markers(*dev)
    vec = vec_t.cpu().numpy()
    want = stats_global(raw.astype(np.float64))
    S, n = float(np.abs(raw).max()), N * T
    assert np.abs(vec[:d] - want['Xmean'].reshape(-1)).max() <= U * n * S
    assert abs(vec[d] - want['Xstd'][0]) / (want['Xstd'][0] + S) <= U * n * d and np.all(vec[d:2 * d] == vec[d])
    # normalised image against the restatement normalised with ITS statistics
    ref = restate_norm(mk, pv, hp)
    sens = DC.sens_of(restate_norm, (mk, pv, hp))[0]
    img, _, _ = b.images_from_markers(*dev, vec_t)
    r = K.ratio(frames_major(img), ref, sens)
    print(f'global_markers T={T} M={M} N={N}: normalised error / sens {r:.3f}')
    assert r <= 4.0, r
    # both layouts, written between guards: the same bits, and not one float outside the image
    for v in (vec_t, None):
        a, buf_a = guarded_write(b, dev, v, False)
        p, buf_p = guarded_write(b, dev, v, True)
        assert torch.equal(a.view(torch.int32), p.transpose(1, 2).contiguous().view(torch.int32))
        for buf in (buf_a, buf_p):
            assert torch.all(buf[:GUARD] == SENTINEL) and torch.all(buf[-GUARD:] == SENTINEL)
            assert not torch.any(buf[GUARD:-GUARD] == SENTINEL)                # every entry of the image was written
        mine = b.images_from_markers(*dev, v)[0]
        assert torch.equal(a.view(torch.int32), mine[:, 0].view(torch.int32))
        assert torch.equal(b.images_from_markers(*dev, v, api_layout=True)[0][:, 0].view(torch.int32), p.view(torch.int32))
    if N > 1:                                                   # chunking and repetition change no bit
        for ch in (1, 2, 5):
            bb = builder(lib, device, M, ch)
            assert np.array_equal(bb.stats_from_markers(*dev).cpu().numpy(), vec)
            assert torch.equal(bb.images_from_markers(*dev, vec_t)[0], img)
        assert np.array_equal(b.stats_from_markers(*dev).cpu().numpy(), vec)


# ---- 5. the fit side ---------------------------------------------------------------------------------------------------------
def fit_loop_image(markers, joints012, Xmean, Xstd):
    """opt_amass_temp.py:366-380 in torch float32: markers [T, M, 3], joints 0-2 of frame 0 [3, 3] -> [T, 3 M]"""
    x_axis = joints012[2] - joints012[1]
    x_axis[-1] = 0
    x_axis = x_axis / torch.norm(x_axis)
    z_axis = torch.tensor([0, 0, 1]).float()
    y_axis = torch.linalg.cross(z_axis, x_axis)
    y_axis = y_axis / torch.norm(y_axis)
    rot = torch.stack([x_axis, y_axis, z_axis], dim=1)
    g = torch.matmul(markers - markers[0, 0], rot)
    clip = g.reshape(g.shape[0], -1).unsqueeze(0)
    return ((clip - Xmean) / Xstd)[0]


def check_fit_side_image(lib, device, T=12):
    clips = DC.synthetic_clips(77, 1, T)
    b = builder(lib, device, 81, models=K.models(lib))
    api, info = b.build(clips, api_layout=True)
    mk, pv, hp = (a.cpu() for a in b._markers(clips, T))
    Xmean, Xstd = torch.from_numpy(info['stats']['Xmean']).float(), torch.from_numpy(info['stats']['Xstd']).float()
    want = fit_loop_image(mk[0], torch.cat([pv[0, :1], hp[0]]), Xmean, Xstd).numpy()
    fixed = lambda *a: restate_norm(*a, stats=info['stats'])
    sens = DC.sens_of(fixed, (mk.numpy(), pv.numpy(), hp.numpy()))[0]
    r = K.ratio(api.cpu().numpy()[0], want, sens)
    print(f'fit side: built image against the fit loop\'s own normalised markers, error / sens {r:.3f}')
    assert r <= 4.0, r


def check_trainer_takes_it(lib, device, T=12):
    from train_epoch_common import sp_trainer
    clips = DC.synthetic_clips(78, 3, T)
    images, _ = builder(lib, device, 67, models=K.models(lib)).build(clips)
    assert tuple(images.shape) == (3, 1, 201, T)
    tr = sp_trainer(lib, device, False, bs=2, d=201, t=T)       # SmoothPriorTrainer(batch=2, H=3 * 67 + 2, W=T - 1 + 16)
    tr.upload_dataset(images)
    assert tr._data.data_ptr() == images.data_ptr()
    log = tr.fit_epoch(torch.tensor([[2, 0]]))
    tr.close()
    print('one fit_epoch step on the built set: losses', log.tolist())
    assert tuple(log.shape) == (1, 3) and bool(torch.isfinite(log).all())


def check_fitter_takes_the_statistics(lib, device, T=12):
    from lemo_amd import synthetic
    from lemo_amd.assets import load_assets, load_vertex_ids
    from lemo_amd.fitting import AmassTemporalFitter
    from lemo_amd.vposer import make_vposer_weights
    clips = DC.synthetic_clips(79, 2, T)
    _, info = builder(lib, device, 81, models=K.models(lib)).build(clips)
    st = info['stats']
    fit = AmassTemporalFitter(synthetic.make_synthetic_smplx(seed=0), make_vposer_weights(2), load_assets()['enc_w'], load_vertex_ids(),
                              st['Xmean'], st['Xstd'], T, device, full_vertices=False, lib=lib)
    assert fit.H == 245 and fit.W == T - 1 + 16
    assert torch.equal(fit._idx['Xmean'].cpu(), torch.from_numpy(st['Xmean']).reshape(-1))
    assert torch.equal(fit._idx['Xstd'].cpu(), torch.from_numpy(st['Xstd']).float())


# ---- 6. validation -----------------------------------------------------------------------------------------------------------
class _PcaModel(K._NoModel):
    use_pca = True


def check_validation(lib, device, monkeypatch):
    launched = []
    for name in ('smplx_pose_fwd', 'clip_repr_stats', 'clip_repr_stats_reduce', 'clip_repr_write', 'lbs_verts_fwd_active'):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    for mode in ('global_joints', 'local_joints', 'local_markers', 'local_markers_4chan', 'markers'):
        with pytest.raises(ValueError):
            SmoothClipImageBuilder({'male': K._NoModel()}, body_mode=mode, device=device, _lib=lib)
    with pytest.raises(ValueError, match='55 regressed joints'):
        SmoothClipImageBuilder({'male': K._NoModel()}, body_mode='global_joints', device=device, _lib=lib)
    with pytest.raises(ValueError):
        SmoothClipImageBuilder({'male': _PcaModel()}, device=device, _lib=lib)
    with pytest.raises(ValueError):                              # the existing class keeps refusing the new name
        ClipImageBuilder({'male': K._NoModel()}, mode='global_markers', _lib=lib)
    good = DC.synthetic_clips(1, 2, 12)
    mod = lambda i, **kw: [dict(c, **kw) if j == i else c for j, c in enumerate(good)]
    cases = [mod(0, poses=good[0]['poses'][:, :150]),
             mod(1, gender='neutral'),
             mod(1, poses=good[1]['poses'][:8], trans=good[1]['trans'][:8]),            # unequal T
             [dict(c, poses=c['poses'][:1], trans=c['trans'][:1]) for c in good],       # T = 1
             [dict(c, poses=np.zeros((257, 156)), trans=np.zeros((257, 3))) for c in good],      # T = 257
             []]
    for M in MS:
        b = builder(lib, device, M)
        assert b.d == 3 * M and b.mode == 'global_markers'
        for clips in cases:
            for call in (b.build, b.compute_stats):
                with pytest.raises(ValueError):
                    call(clips)
        other = 3 * (M + 1)
        for stats in (dict(Xmean=np.zeros((1, 1, other)), Xstd=np.ones(other)),          # local_markers' statistics
                      dict(Xmean=np.zeros((1, 1, 3 * M)), Xstd=np.ones(other)),
                      dict(Xmean_local=np.zeros(other + 4), Xstd_local=np.ones(other + 4)),      # the infilling prior's
                      dict(Xmean=np.zeros((1, 1, 3 * (148 - M))), Xstd=np.ones(3 * (148 - M)))):   # the other marker set's
            with pytest.raises(ValueError):
                b.build(good, stats=stats)
    assert launched == []
    monkeypatch.undo()
    # the native layer refuses on its own
    d = _hip.ClipReprDesc(markers=1, pelvis=1, hips0=1, n_clips=1, T=30, M=67, mode=2, fps=30.0, image=1, stats_part=1)
    for T, M in ((257, 67), (1, 67), (30, 60), (30, 68), (30, 84)):
        d.T, d.M = T, M
        assert lib.clip_repr_write(d, None) == 10001 and lib.clip_repr_stats(d, None) == 10001
        assert lib.clip_repr_stats_reduce(1, 1, T, M, 2, 1, None) == 10001
    d.T, d.M = 30, 67
    for mode in (3, -1):
        d.mode = mode
        assert lib.clip_repr_write(d, None) == 10002 and lib.clip_repr_stats(d, None) == 10002
        assert lib.clip_repr_stats_reduce(1, 1, 30, 67, mode, 1, None) == 10002
    assert lib.clip_repr_stats_k(67, 2) == 201 + 8 and lib.clip_repr_stats_k(81, 2) == 243 + 8
