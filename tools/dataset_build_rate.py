"""Clips per second of ``ClipImageBuilder.build`` / ``SmoothClipImageBuilder.build`` next to what a user had before them: a
per-clip loop of the module forward, torch canonicalisation (and, for ``local_markers_4chan``, contact labels and
``markers.get_local_markers_4chan``) and torch statistics + normalisation of the same representation.

    python tools/dataset_build_rate.py [--mode local_markers_4chan|local_markers|global_markers|all] [--clips 2048] [--frames 120]
                                       [--loop-clips 256] [--out profiles/dataset_build_rate.txt]

``global_markers`` (the shipped smoothness prior's representation) runs with hands, 81 markers, like the reference's default.

Both on the same GPU, synthetic SMPL-X models (full size) and seeded AMASS-shaped clips, device events, median of 5 runs
after one warm-up.  The loop is timed on ``--loop-clips`` clips (its cost is per clip).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd import synthetic                                   # noqa: E402
from lemo_amd.assets import load_vertex_ids                      # noqa: E402
from lemo_amd.body_model import SMPLX                            # noqa: E402
from lemo_amd.dataset import ClipImageBuilder, SmoothClipImageBuilder    # noqa: E402
from lemo_amd.markers import get_local_markers_4chan             # noqa: E402


def make_clips(n, T, seed=0):
    rng = np.random.default_rng(seed)
    clips = []
    for i in range(n):
        poses = np.cumsum(rng.standard_normal((T, 156)) * 0.01, 0) + rng.standard_normal(156) * 0.2
        trans = np.cumsum(rng.standard_normal((T, 3)) * 0.01, 0)
        clips.append(dict(poses=poses, trans=trans, betas=rng.standard_normal(16) * 0.5, gender='male' if i % 2 == 0 else 'female',
                          mocap_framerate=120))
    return clips


FEET = [16, 47, 30, 60]


def median_ms(fn, runs=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def loop(models, clips, ids, dev, fps=30.0, mode='local_markers_4chan'):
    """what a user of the project had before the builder: its pieces, one clip at a time"""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    imgs = []
    for c in clips:
        T = len(c['poses'])
        p = f(c['poses'])
        out = models[c['gender']](betas=f(np.tile(c['betas'][:10], (T, 1))), global_orient=p[:, :3], body_pose=p[:, 3:66],
                                  left_hand_pose=p[:, 66:111], right_hand_pose=p[:, 111:], transl=f(c['trans']))
        joints, markers = out.joints.detach(), out.vertices.detach()[:, ids]
        # first-frame frame: the hip line, flattened, becomes the x axis; a turn about the up axis by its angle
        origin, hip = joints[0, 0], joints[0, 2, :2] - joints[0, 1, :2]
        co, si = (hip / hip.norm()).unbind()

        def turn(p):
            q = p - origin
            return torch.stack([co * q[..., 0] + si * q[..., 1], co * q[..., 1] - si * q[..., 0], q[..., 2]], -1)
        if mode != 'local_markers_4chan':
            # the smoothness loader's two marker representations: markers from marker 0 of frame 0; with the pelvis row in front
            # and relative to it (local_markers), or alone (global_markers)
            pelvis = turn(joints[:, 0:1])
            origin = markers[0, 0]
            markers = turn(markers)
            body = torch.cat([pelvis, markers - pelvis], 1) if mode == 'local_markers' else markers
            imgs.append(body.reshape(T, -1))
            continue
        pelvis, markers = turn(joints[:, 0:1]), turn(markers)
        # contact: a foot marker is low (within 10 cm of the clip's lowest marker) and, except in the last frame, slower than 0.22 m/s
        feet = markers[:, FEET]
        lbl = (feet[..., 2] < markers[..., 2].min() + 0.10).float()
        lbl[:-1] *= ((feet[1:] - feet[:-1]).norm(dim=-1) * fps < 0.22).float()
        img, _ = get_local_markers_4chan(torch.cat([pelvis, markers], 1), lbl)
        imgs.append(img)
    x = torch.stack(imgs).double()
    if mode != 'local_markers_4chan':
        mean, std = x.mean(dim=(0, 1)), torch.ones(x.shape[-1], dtype=x.dtype, device=x.device) * x.std(unbiased=False)
        if mode == 'local_markers':
            x[..., :3] = (x[..., :3] - mean[:3]) / x[..., :3].std(unbiased=False)
        else:
            x = (x - mean) / std
        return x.float().permute(0, 2, 1).unsqueeze(1).contiguous()
    mean = x[:, 0].mean(dim=(0, 1))
    mean[-4:] = 0
    std = torch.ones_like(mean) * x[:, 0].std(unbiased=False)
    std[-4:] = 1
    x[:, 0] = (x[:, 0] - mean) / std
    x[:, 1:3] = (x[:, 1:3] - x[:, 1:3].mean()) / x[:, 1:3].std(unbiased=False)
    x[:, 3] = (x[:, 3] - x[:, 3].mean()) / x[:, 3].std(unbiased=False)
    return x.float().permute(0, 1, 3, 2).contiguous()


def measure(mode, models, clips, a, dev):
    hand = mode == 'global_markers'
    ids = torch.from_numpy(np.asarray(load_vertex_ids()['markers81' if hand else 'markers67'])).to(dev)
    if mode == 'global_markers':
        b = SmoothClipImageBuilder(models, with_hand=True, chunk=a.chunk, device=dev)
    else:
        b = ClipImageBuilder(models, mode=mode, chunk=a.chunk, device=dev)
    ms_b, all_b = median_ms(lambda: b.build(clips))
    few = clips[:a.loop_clips]
    ms_l, all_l = median_ms(lambda: loop(models, few, ids, dev, mode=mode))
    T = a.frames
    mk, pv, hp = b._markers(clips, T)
    ms_k, _ = median_ms(lambda: b.images_from_markers(mk, pv, hp, b.stats_from_markers(mk, pv, hp)))
    pieces = ('module forward, torch canonicalisation + labels, get_local_markers_4chan, torch statistics' if mode == 'local_markers_4chan'
              else 'module forward, torch canonicalisation, torch statistics')
    return [f'{torch.cuda.get_device_name(0)}; T = {T}, {b.M} markers, mode {mode}, median of 5 runs (device events), host work included',
            f'{type(b).__name__}.build, {a.clips} clips, chunk {a.chunk}: {ms_b:.1f} ms = {a.clips / ms_b * 1e3:.0f} clips/s   (runs: {", ".join(f"{t:.1f}" for t in all_b)})',
            f'  of which statistics + write passes on resident markers: {ms_k:.2f} ms = {a.clips / ms_k * 1e3:.0f} clips/s',
            f'per-clip loop ({pieces}), {len(few)} clips: '
            f'{ms_l:.1f} ms = {len(few) / ms_l * 1e3:.0f} clips/s   (runs: {", ".join(f"{t:.1f}" for t in all_l)})']


MODES = ('local_markers_4chan', 'local_markers', 'global_markers')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', default='local_markers_4chan', choices=MODES + ('all',))
    ap.add_argument('--clips', type=int, default=2048)
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--loop-clips', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    models = {g: SMPLX(synthetic.make_synthetic_smplx(seed=s), gender=g, use_pca=False, flat_hand_mean=True).to(dev)
              for g, s in (('male', 0), ('female', 1))}
    clips = make_clips(a.clips, a.frames)
    lines = []
    for mode in (MODES if a.mode == 'all' else (a.mode,)):
        lines += measure(mode, models, clips, a, dev) + ['']
    lines = lines[:-1]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
