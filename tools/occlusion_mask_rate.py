"""Frames per second of ``OcclusionMasker`` (lemo_amd/occlusion.py) and the one-off cost of ``SceneDepth``.

    python tools/occlusion_mask_rate.py [--frames 1000] [--points 92] [--scene-cells 500] [--out profiles/occlusion_mask_rate.txt]

The body is the SMPL-X-shaped synthetic model (V = 10475, F = 20908, faces redrawn as small triangles, ``synthetic.local_faces``)
in ``--frames`` poses 2.5 m from PROX's camera; the points are the first 25 joints and the 67 markers.  The scene is a bumpy panel
of 2 x cells^2 triangles in front of its left half plus two floor triangles that cross the near plane, at 1920 x 1080.  Device events, median of 5
runs after one warm-up.  There is no earlier figure to compare with: the file records what was measured and on which GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd import synthetic                                   # noqa: E402
from lemo_amd.assets import load_vertex_ids                      # noqa: E402
from lemo_amd.body_model import create                           # noqa: E402
from lemo_amd.occlusion import OcclusionMasker, SceneDepth       # noqa: E402


def wall(cells, seed=0):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(-3, 0, cells + 1), np.linspace(-1.5, 1.5, cells + 1), indexing='ij')
    gz = 2.0 + 0.3 * np.sin(3 * gx) * np.cos(2 * gy) + rng.standard_normal(gx.shape) * 0.002
    v = np.stack([gx, gy, gz], -1).reshape(-1, 3)
    idx = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate([np.stack([a, c, b], -1), np.stack([a, d, c], -1)])          # counter-clockwise as the camera sees them
    floor = np.array([[-4, 1.2, -1.0], [4, 1.2, -1.0], [4, 1.2, 6.0], [-4, 1.2, 6.0]])
    f = np.concatenate([f, np.array([[0, 1, 2], [0, 2, 3]]) + len(v)])
    return np.concatenate([v, floor]).astype(np.float32), f.astype(np.int32)


def timed(fn, runs=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--points', type=int, default=92)
    ap.add_argument('--scene-cells', type=int, default=500)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'occlusion_mask_rate.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a rate is measured on the GPU'
    dev = torch.device('cuda:0')
    T, P = args.frames, args.points
    sv, sf = wall(args.scene_cells)
    svd, sfd = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    ms_scene, runs_scene = timed(lambda: SceneDepth(svd, sfd))
    scene = SceneDepth(svd, sfd)
    model = synthetic.make_synthetic_smplx(seed=0)
    model['f'] = synthetic.local_faces(model['v_template'], model['f'].shape[0])
    B = 100
    bm = create(model, batch_size=B).to(dev)
    g = torch.Generator().manual_seed(0)
    verts, joints = [], []
    with torch.no_grad():
        for lo in range(0, T, B):
            r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
            transl = (torch.tensor([0.0, 0.0, 2.5]) + torch.randn(B, 3, generator=g) * 0.1).to(dev)
            out = bm(global_orient=r(B, 3, k=0.3), body_pose=r(B, 63, k=0.15), transl=transl, betas=r(B, 10, k=0.5))
            verts.append(out.vertices); joints.append(out.joints[:, :25])
    verts, joints = torch.cat(verts)[:T].contiguous(), torch.cat(joints)[:T]
    ids = torch.from_numpy(np.asarray(load_vertex_ids()['markers67'], np.int64)).to(dev)
    points = torch.cat([joints, verts[:, ids]], 1)[:, :P].contiguous()
    masker = OcclusionMasker(scene, bm.faces)
    ms, runs = timed(lambda: masker(verts, points))
    mask = masker(verts, points)
    fmt = lambda rs: ', '.join(f'{v:.2f}' for v in rs)
    lines = [f'{torch.cuda.get_device_name(0)}; 1920 x 1080, median of 5 runs after one warm-up (device events)',
             f'SceneDepth, {len(sf)} triangles ({len(sv)} vertices), two of them across the near plane: {ms_scene:.2f} ms   (runs: {fmt(runs_scene)})',
             f'OcclusionMasker, T = {T} frames, V = {verts.shape[1]}, F = {bm.faces.shape[0]}, P = {P} points: {ms:.2f} ms = {T / ms * 1e3:.0f} frames/s   (runs: {fmt(runs)})',
             f'  scene covers {float((scene.depth != 0).float().mean()):.3f} of the image; {float(1 - mask.mean()):.3f} of the points occluded']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
