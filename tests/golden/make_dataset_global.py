"""Emit the fixture of the ``global_markers`` dataset-builder tests: the reference's smoothness loader
(loader/train_loader_smooth.py, imported from where it lies; nothing is copied) in its default mode, on the clips of
make_dataset.py.

Run ONLY in the build container (needs the reference tree; it never travels to the GPU box):

    python tests/golden/make_dataset_global.py

The models, the served ``smplx.create`` and the clips are make_dataset.py's (imported from it; the clips are asserted to be
the ones dataset_repr_inputs.npz holds).  For ``with_hand=False`` (67 markers) and ``with_hand=True`` (81) and both groups
(4 clips of 30 frames, 2 of 120) ``create_body_repr`` runs in mode ``global_markers`` unnormalised, as the train split and
as the test split (asserted equal to the train split).  Written, in two files of under 1 MiB each:

  dataset_repr_global.npz       g{T}_raw{M} [N, T, 3 M] float32 the unnormalised images; g{T}_stats{M}_Xmean (1, 1, 3 M) float32 and
                                g{T}_stats{M}_Xstd (3 M,) float64, the statistics the loader saved; g{T}_sens [2] (M = 67, 81);
                                g{T}_stats_f32_gap [2, 2] (M; Xmean, Xstd); g{T}_m81_extra [N, T, 14, 3] float32, the reference's
                                world-frame markers 67-80 of the 81-marker set (its first 67 are the 67-marker set, asserted; those,
                                the pelvis and the hips are m{T}_* of dataset_repr_inputs.npz, asserted equal)
  dataset_repr_global_norm.npz  g{T}_norm{M} [N, T, 3 M] float32: the normalised images as ``__getitem__`` hands them to the trainer
                                (permuted back to frame-major rows)

``g{T}_sens``: the largest change of the reference's normalised image when every float32 the model hands the loader is moved by
one ulp, over 8 seeded perturbations (the definition of the existing ``sens``).  ``g{T}_stats_f32_gap``: the largest distance
between the statistics the reference computed -- float32 numpy reductions, its array is float32 -- and float64 statistics of
that same array.
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
sys.path.insert(0, HERE)

import make_dataset as MD                                     # noqa: E402  (puts the repository and tests/ on sys.path)
import dataset_common as DC                                   # noqa: E402
import ref_harness as RH                                      # noqa: E402
from lemo_amd import synthetic                                # noqa: E402
from oracle import lemo_oracle as O                           # noqa: E402

MODE = 'global_markers'


def run(cls, clips, T, with_hand, normalize, split='train', rng=None):
    ld = cls(clip_seconds=T // 30, clip_fps=30, normalize=normalize, split=split, mode=MODE)
    ld.data_dict_list = [dict(c) for c in clips]
    ld.n_samples = len(clips)
    MD.ServedModel.rng, MD.ServedModel.log = rng, []
    ld.create_body_repr(with_hand=with_hand, smplx_model_path=None)
    MD.ServedModel.rng = None
    return ld, list(MD.ServedModel.log)


def main():
    RH.install_stubs()
    sys.modules['smplx'].create = MD.create
    try:
        import tqdm                                            # noqa: F401
    except ImportError:
        t = types.ModuleType('tqdm'); t.tqdm = lambda x, *a, **k: x
        sys.modules['tqdm'] = t
    for g, seed in MD.MODEL_SEED.items():
        MD.ServedModel.so[g] = O.SmplxOracle(synthetic.make_synthetic_smplx(seed=seed), use_pca=False, flat_hand_mean=True)
    inputs = DC.load_fixture()
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.makedirs(os.path.join(tmp, 'loader')); os.makedirs(os.path.join(tmp, 'preprocess_stats'))
    for f in ('SSM2.json', 'SSM2_withhand.json'):
        shutil.copy(os.path.join(MD.REF, 'loader', f), os.path.join(tmp, 'loader', f))
    os.chdir(tmp)
    G, Nn = {}, {}
    try:
        from loader.train_loader_smooth import TrainLoader as Smooth
        from lemo_amd.assets import load_vertex_ids
        ids = {}
        for M, f in ((67, 'SSM2.json'), (81, 'SSM2_withhand.json')):
            with open('loader/' + f) as fh:
                ids[M] = list(json.load(fh)['markersets'][0]['indices'].values())
            assert list(load_vertex_ids()[f'markers{M}']) == ids[M]
        assert ids[81][:67] == ids[67]
        for T, n, seed in MD.GROUPS:
            clips = MD.pick_clips(seed, n, T, ids[67])
            assert np.array_equal(np.stack([c['poses'] for c in clips]).astype(np.float32), inputs[f'c{T}_poses'])
            assert np.array_equal(np.stack([c['trans'] for c in clips]).astype(np.float32), inputs[f'c{T}_trans'])
            sens, gap = np.zeros(2), np.zeros((2, 2))
            for k, M in enumerate((67, 81)):
                hand = M == 81
                ld, log = run(Smooth, clips, T, hand, False)
                raw = ld.clip_img_list
                assert raw.dtype == np.float32 and raw.shape == (n, T, 3 * M)
                markers = np.stack([v[:, ids[M]].numpy() for v, _ in log])
                assert np.array_equal(markers[:, :, :67], inputs[f'm{T}_markers'])
                assert np.array_equal(np.stack([j[:, 0].numpy() for _, j in log]), inputs[f'm{T}_pelvis'])
                assert np.array_equal(np.stack([j[0, 1:3].numpy() for _, j in log]), inputs[f'm{T}_hips0'])
                if hand:
                    G[f'g{T}_m81_extra'] = markers[:, :, 67:]
                ld, _ = run(Smooth, clips, T, hand, True, 'train')
                train = ld.clip_img_list
                name = 'preprocess_stats/preprocess_stats_smooth{}_{}.npz'.format('_withHand' if hand else '', MODE)
                stats = dict(np.load(name))
                assert stats['Xmean'].shape == (1, 1, 3 * M) and stats['Xmean'].dtype == np.float32
                assert stats['Xstd'].shape == (3 * M,) and stats['Xstd'].dtype == np.float64 and np.all(stats['Xstd'] == stats['Xstd'][0])
                item = torch.stack([ld[i][0] for i in range(n)])                         # [N, 1, d, T] float32
                assert item.dtype == torch.float32 and tuple(item.shape) == (n, 1, 3 * M, T)
                norm = item[:, 0].permute(0, 2, 1).contiguous().numpy()
                assert np.array_equal(norm, train.astype(np.float32))
                ld, _ = run(Smooth, clips, T, hand, True, 'test')
                assert np.array_equal(ld.clip_img_list, train)
                G[f'g{T}_raw{M}'], Nn[f'g{T}_norm{M}'] = raw, norm
                G[f'g{T}_stats{M}_Xmean'], G[f'g{T}_stats{M}_Xstd'] = stats['Xmean'], stats['Xstd']
                r64 = raw.astype(np.float64)
                gap[k] = [np.abs(r64.mean(axis=1).mean(axis=0) - stats['Xmean'].reshape(-1)).max(), abs(r64.std() - stats['Xstd'][0])]
                rng = np.random.default_rng(3000 + T + M)
                for _ in range(8):
                    ld, _ = run(Smooth, clips, T, hand, True, 'train', rng=rng)
                    sens[k] = max(sens[k], float(np.abs(ld.clip_img_list.astype(np.float64) - train).max()))
            G[f'g{T}_sens'], G[f'g{T}_stats_f32_gap'] = sens, gap
            print(f'T={T} global_markers sens (67, 81)', sens, ' statistics float32 gap (Xmean, Xstd)', gap.tolist())
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    for name, d in (('dataset_repr_global.npz', G), ('dataset_repr_global_norm.npz', Nn)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        print(name, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    torch.set_num_threads(16)
    main()
