"""Emit the fixtures of the dataset-builder tests: the reference's own loaders (loader/train_loader_infill.py and
loader/train_loader_smooth.py, imported from where they lie; nothing is copied) run on seeded AMASS-shaped clips.

Run ONLY in the build container (needs the reference tree; it never travels to the GPU box):

    python tests/golden/make_dataset.py

``smplx.create`` is served by ``ref_harness.RefSmplx`` on the seeded synthetic models (male: seed 0, female: seed 1) with
``use_pca=False, flat_hand_mean=True``; the loaders run from a temporary working directory that holds ``loader/SSM2*.json``
and ``preprocess_stats/``.  For both modes (``local_markers_4chan`` of the infilling loader, ``local_markers`` of the
smoothness loader) and both groups (4 clips of 30 frames, 2 of 120) ``create_body_repr`` runs unnormalised, as the train
split and as the test split (asserted equal to the train split).  Written, in three files of under 1 MiB each:

  dataset_repr.npz          a{T}_raw   [N, T-1, 208] float64 channel 0 of the unnormalised 4chan images, a{T}_raw_g [N, 3, T-1]
                            one row of channels 1-3, a{T}_body [N, T, 68, 3] the canonicalised pelvis + markers (float32, read off the
                            loader's own run: what its torch.cat returned), a{T}_stats_* the statistics it saved
  dataset_repr_inputs.npz   c{T}_poses / trans / betas / gender: the clips; m{T}_markers / pelvis / hips0: the reference's float32
                            world-frame markers, joint 0 and joints 1-2 of frame 0; a{T}_norm / a{T}_norm_g: the normalised images
                            as float32 (what ``__getitem__`` hands the trainer); a{T}_sens [4], s{T}_sens [2]
  dataset_repr_smooth.npz   s{T}_raw [N, T, 204] float32, s{T}_norm3 [N, T, 3] (the only normalised columns), s{T}_stats_*;
                            div_* what ``divide_clip`` makes of dataset_common.amass_sequences()

``sens``: per channel, the largest change of the reference's normalised image when every float32 the model hands the loader
is moved by one ulp, over 8 seeded perturbations.  The generator asserts that no foot speed lies within 1e-4 of 0.22 and no
foot height within 1e-4 of its threshold, under which the labels are exact.
"""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import dataset_common as DC                                   # noqa: E402
import ref_harness as RH                                      # noqa: E402
from lemo_amd import synthetic                                # noqa: E402
from oracle import lemo_oracle as O                           # noqa: E402

GROUPS = ((30, 4, 301), (120, 2, 302))                        # (T, clips, seed)
MODEL_SEED = {'male': 0, 'female': 1}


class ServedModel:
    """what ``smplx.create`` returns here: RefSmplx per gender with the outputs cached per input (the perturbation runs ask
    for the same clips again) and, when ``ServedModel.rng`` is set, every float32 of the output moved by one ulp"""
    so = {}
    cache = {}
    rng = None
    log = []

    def __init__(self, gender):
        self.gender = gender

    def to(self, device):
        return self

    def __call__(self, return_verts=True, **p):
        key = (self.gender, p['transl'].numpy().tobytes(), p['global_orient'].numpy().tobytes())
        if key not in ServedModel.cache:
            T = p['transl'].shape[0]
            m = RH.RefSmplx(ServedModel.so[self.gender], batch_size=T)
            with torch.no_grad():
                out = m(**p)
            ServedModel.cache[key] = (out.vertices.clone(), out.joints.clone())
        v, j = (t.clone() for t in ServedModel.cache[key])
        if ServedModel.rng is not None:
            v = torch.from_numpy(DC.perturb_ulp(v.numpy(), ServedModel.rng))
            j = torch.from_numpy(DC.perturb_ulp(j.numpy(), ServedModel.rng))
        ServedModel.log.append((v.clone(), j.clone()))
        return types.SimpleNamespace(vertices=v, joints=j)


def create(model_path, model_type='smplx', gender='male', **kw):
    assert kw['use_pca'] is False and kw['flat_hand_mean'] is True
    return ServedModel(gender)


def run(cls, clips, mode, T, normalize, split='train', rng=None):
    ld = cls(clip_seconds=T // 30, clip_fps=30, normalize=normalize, split=split, mode=mode)
    ld.data_dict_list = [dict(c) for c in clips]
    ld.n_samples = len(clips)
    ServedModel.rng, ServedModel.log = rng, []
    ld.create_body_repr(with_hand=False, smplx_model_path=None)
    ServedModel.rng = None
    return np.asarray(ld.clip_img_list), list(ServedModel.log)


def pick_clips(seed, n, T, marker_ids):
    """seeded clips in which some foot marker is in contact for part of the time (the synthetic body has no feet to stand on:
    most random orientations give no contact at all, which would leave the label logic untested)"""
    clips = []
    for i in range(n):
        for k in range(200):
            c = DC.synthetic_clips(seed + 1000 * i + k, 1, T)[0]
            c['gender'] = 'male' if i % 2 == 0 else 'female'
            f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
            out = ServedModel(c['gender'])(transl=f(c['trans']), global_orient=f(c['poses'][:, :3]), body_pose=f(c['poses'][:, 3:66]),
                                           left_hand_pose=f(c['poses'][:, 66:111]), right_hand_pose=f(c['poses'][:, 111:]),
                                           betas=f(np.tile(c['betas'][:10], (T, 1))))
            _, _, lbl, body = DC.raw_4chan(out.vertices[:, marker_ids].numpy(), out.joints[:, 0].numpy(), out.joints[0, 1:3].numpy())
            speed, height, thr = DC.foot_margins(body[:, 1:])
            if 0.03 < lbl.mean() < 0.9 and np.abs(speed - 0.22).min() > 3e-4 and np.abs(height - thr).min() > 3e-4:
                break
        else:
            raise RuntimeError('no clip with contact found')
        clips.append(c)
    return clips


class TorchTap:
    """stands in for ``torch`` inside the loader module: everything is torch's own, and what ``cat`` returns is kept, so that
    the body the loader itself canonicalised (pelvis + markers, [T, 68, 3]) can be read off its own run"""
    kept = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def cat(self, *a, **k):
        out = torch.cat(*a, **k)
        TorchTap.kept.append(out.detach().clone())
        return out


def main():
    RH.install_stubs()
    sys.modules['smplx'].create = create
    try:
        import tqdm                                            # noqa: F401
    except ImportError:
        t = types.ModuleType('tqdm'); t.tqdm = lambda x, *a, **k: x
        sys.modules['tqdm'] = t
    for g, seed in MODEL_SEED.items():
        ServedModel.so[g] = O.SmplxOracle(synthetic.make_synthetic_smplx(seed=seed), use_pca=False, flat_hand_mean=True)
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.makedirs(os.path.join(tmp, 'loader')); os.makedirs(os.path.join(tmp, 'preprocess_stats'))
    for f in ('SSM2.json', 'SSM2_withhand.json'):
        shutil.copy(os.path.join(REF, 'loader', f), os.path.join(tmp, 'loader', f))
    os.chdir(tmp)
    try:
        from loader.train_loader_infill import TrainLoader as Infill
        from loader.train_loader_smooth import TrainLoader as Smooth
        sys.modules[Infill.__module__].torch = TorchTap()
        with open('loader/SSM2.json') as f:
            marker_ids = list(json.load(f)['markersets'][0]['indices'].values())
        from lemo_amd.assets import load_vertex_ids
        assert list(load_vertex_ids()['markers67']) == marker_ids
        A, B, S = {}, {}, {}
        for T, n, seed in GROUPS:
            clips = pick_clips(seed, n, T, marker_ids)
            B[f'c{T}_poses'] = np.stack([c['poses'] for c in clips]).astype(np.float32)
            B[f'c{T}_trans'] = np.stack([c['trans'] for c in clips]).astype(np.float32)
            B[f'c{T}_betas'] = np.stack([c['betas'] for c in clips]).astype(np.float32)
            B[f'c{T}_gender'] = np.array([c['gender'] for c in clips])
            # ---- infilling loader, local_markers_4chan
            TorchTap.kept = []
            raw, log = run(Infill, clips, 'local_markers_4chan', T, False)
            body = np.stack([t.numpy() for t in TorchTap.kept if tuple(t.shape) == (T, 68, 3)])
            assert body.shape == (n, T, 68, 3) and body.dtype == np.float32
            assert raw.dtype == np.float64 and raw.shape == (n, 4, T - 1, 208)
            B[f'm{T}_markers'] = np.stack([v[:, marker_ids].numpy() for v, _ in log])
            B[f'm{T}_pelvis'] = np.stack([j[:, 0].numpy() for _, j in log])
            B[f'm{T}_hips0'] = np.stack([j[0, 1:3].numpy() for _, j in log])
            frac = []
            for i in range(n):
                img, _, lbl = DC.raw_4chan_from_body(body[i])
                assert np.abs(img - raw[i]).max() < 1e-12, np.abs(img - raw[i]).max()
                assert np.array_equal(lbl[:-1], raw[i, 0, :, -4:])
                speed, height, thr = DC.foot_margins(body[i, :, 1:])
                assert np.abs(speed - 0.22).min() > 1e-4 and np.abs(height - thr).min() > 1e-4, (np.abs(speed - 0.22).min(), np.abs(height - thr).min())
                frac.append(lbl.mean())
            print(f'T={T} 4chan: contact fraction per clip', np.round(frac, 3))
            assert all(np.array_equal(raw[:, c, :, :1].repeat(208, -1), raw[:, c]) for c in (1, 2, 3))
            train, _ = run(Infill, clips, 'local_markers_4chan', T, True, 'train')
            stats = dict(np.load('preprocess_stats/preprocess_stats_infill_local_markers_4chan.npz'))
            test, _ = run(Infill, clips, 'local_markers_4chan', T, True, 'test')
            assert np.array_equal(train, test)
            mine = DC.stats_4chan(raw)
            assert all(np.array_equal(mine[k], stats[k]) for k in stats), 'the restated statistics are not the loader\'s'
            assert np.array_equal(DC.normalise_4chan(raw, stats), train)
            A[f'a{T}_raw'], A[f'a{T}_raw_g'], A[f'a{T}_body'] = raw[:, 0], raw[:, 1:, :, 0], body.astype(np.float32)
            for k, v in stats.items():
                A[f'a{T}_stats_{k}'] = v
            B[f'a{T}_norm'], B[f'a{T}_norm_g'] = train[:, 0].astype(np.float32), train[:, 1:, :, 0].astype(np.float32)
            sens = np.zeros(4)
            rng = np.random.default_rng(1000 + T)
            for _ in range(8):
                got, _ = run(Infill, clips, 'local_markers_4chan', T, True, 'train', rng=rng)
                assert np.array_equal(got[:, 0, :, -4:], train[:, 0, :, -4:])
                sens = np.maximum(sens, np.abs(got - train).max(axis=(0, 2, 3)))
            B[f'a{T}_sens'] = sens
            print(f'T={T} 4chan sens', sens)
            # ---- smoothness loader, local_markers
            raw, log = run(Smooth, clips, 'local_markers', T, False)
            assert raw.dtype == np.float32 and raw.shape == (n, T, 204)
            train, _ = run(Smooth, clips, 'local_markers', T, True, 'train')
            stats = dict(np.load('preprocess_stats/preprocess_stats_smooth_local_markers.npz'))
            test, _ = run(Smooth, clips, 'local_markers', T, True, 'test')
            assert np.array_equal(train, test) and np.array_equal(train[:, :, 3:], raw[:, :, 3:])
            mine = DC.stats_smooth(raw)
            assert all(np.array_equal(mine[k], stats[k]) for k in stats)
            assert np.array_equal(DC.normalise_smooth(raw, stats), train)
            S[f's{T}_raw'], S[f's{T}_norm3'] = raw, train[:, :, :3]
            for k, v in stats.items():
                S[f's{T}_stats_{k}'] = v
            sens = np.zeros(2)
            rng = np.random.default_rng(2000 + T)
            for _ in range(8):
                got, _ = run(Smooth, clips, 'local_markers', T, True, 'train', rng=rng)
                dlt = np.abs(got.astype(np.float64) - train)
                sens = np.maximum(sens, [dlt[:, :, :3].max(), dlt[:, :, 3:].max()])
            B[f's{T}_sens'] = sens
            print(f'T={T} smooth sens', sens)
        # ---- divide_clip on tiny files
        seqs = DC.amass_sequences()
        for i, s in enumerate(seqs):
            os.makedirs(f'amass/DS/subj{i}')
            np.savez(f'amass/DS/subj{i}/seq{i}_poses.npz', **s)
        ld = Infill(clip_seconds=1, clip_fps=30, mode='local_markers_4chan')
        ld.read_data(['DS'], 'amass')
        recs = []
        for c in ld.data_dict_list:
            src = [i for i, s in enumerate(seqs) if np.array_equal(s['betas'], c['betas'])]
            assert len(src) == 1
            start = int(np.nonzero((seqs[src[0]]['poses'] == c['poses'][0]).all(1))[0][0])
            recs.append([src[0], start, len(c['poses']), int(c['mocap_framerate']), float(c['poses'].sum()), float(c['trans'].sum())])
        S['div_clips'] = np.asarray(sorted(recs), np.float64)
        S['div_gender'] = np.array([str(seqs[int(r[0])]['gender']) for r in sorted(recs)])
        print('divide_clip:', len(recs), 'clips')
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    for name, d in (('dataset_repr.npz', A), ('dataset_repr_inputs.npz', B), ('dataset_repr_smooth.npz', S)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        print(name, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    torch.set_num_threads(16)
    main()
