"""Time per frame of ``BodyRenderer`` (lemo_amd/render.py), pass by pass, next to the parent's only yardstick: one
``occlusion.render_depth`` call per frame on the same frames.

    python tools/render_rate.py [--frames 100] [--chunk 16] [--out profiles/render_rate.txt]

The body is the SMPL-X-shaped synthetic model (V = 10475, F = 20908, faces redrawn as small triangles, ``synthetic.local_faces``)
in ``--frames`` poses 1.3 m from PROX's camera, where it fills a third of the 1920 x 1080 image; the background is one shared uint8
frame, the points are the first 25 joints.  The passes are timed through the C entry points on ``--chunk`` frames at a time
(lemo_render_ids holds the depth pass and the id pass: two walks over the triangles), the whole call through ``BodyRenderer``.
Device events around the repeated launches, median of 5 runs after one warm-up.  No rate is asserted anywhere: the file records what
was measured and on which GPU.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd import _hip, synthetic                             # noqa: E402
from lemo_amd._hip import ptr                                    # noqa: E402
from lemo_amd.body_model import create                           # noqa: E402
from lemo_amd.occlusion import PROX_RENDER, render_depth         # noqa: E402
from lemo_amd.render import BodyRenderer                         # noqa: E402


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
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--chunk', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'render_rate.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a rate is measured on the GPU'
    dev = torch.device('cuda:0')
    lib = _hip.get_lib()
    B, n = args.frames, min(args.frames, args.chunk)
    W, H = PROX_RENDER['W'], PROX_RENDER['H']
    model = synthetic.make_synthetic_smplx(seed=0)
    model['f'] = synthetic.local_faces(model['v_template'], model['f'].shape[0])
    bm = create(model, batch_size=B).to(dev)
    g = torch.Generator().manual_seed(0)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
    transl = (torch.tensor([-0.2, 0.0, 1.3]) + torch.randn(B, 3, generator=g) * torch.tensor([0.1, 0.03, 0.05])).to(dev)
    with torch.no_grad():
        out = bm(global_orient=r(B, 3, k=0.3), body_pose=r(B, 63, k=0.15), transl=transl, betas=r(B, 10, k=0.5))
    verts = out.vertices.contiguous()
    j = out.joints[:, :25]
    joints2d = torch.stack([PROX_RENDER['fx'] * j[..., 0] / j[..., 2] + PROX_RENDER['cx'],
                            PROX_RENDER['fy'] * j[..., 1] / j[..., 2] + PROX_RENDER['cy']], -1).contiguous()
    bg = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    rend = BodyRenderer(bm.faces, chunk=args.chunk)
    V = verts.shape[1]
    faces, start, face, nnz = rend.topology.on(dev, V)
    F = faces.shape[0]
    keys = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    ids = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    normals = torch.empty(n, V, 3, device=dev)
    img = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    s = lib.stream(dev)
    cam, shade = C.byref(rend._cam), C.byref(rend._shade)
    v = verts[:n]
    passes = [
        ('vertex normals', lambda: lib.check(lib.vertex_normals(ptr(v), n, V, ptr(faces), F, ptr(start), ptr(face), nnz, ptr(normals), None, s))),
        ('depth pass + id pass', lambda: lib.check(lib.render_ids(ptr(v), n, V, ptr(faces), F, cam, ptr(keys), ptr(ids), None, s))),
        ('resolve over a shared uint8 frame', lambda: lib.check(lib.render_resolve(ptr(v), ptr(normals), n, V, ptr(faces), F, cam, ptr(ids), shade,
                                                                                  ptr(bg), 1, 1, ptr(img), None, None, s))),
        ('points, 25 of radius 2', lambda: lib.check(lib.render_points(ptr(joints2d[:n]), n, 25, 2, W, H, 0xFF0000, ptr(img), s))),
    ]
    fmt = lambda rs: ', '.join(f'{x:.2f}' for x in rs)
    lines = [f'{torch.cuda.get_device_name(0)}; {W} x {H}, V = {V}, F = {F}, median of 5 runs after one warm-up (device events)',
             f'passes on {n} frames per set of launches:']
    for what, fn in passes:
        ms, runs = timed(fn)
        lines.append(f'  {what}: {ms / n:.3f} ms per frame   (runs of {n} frames, ms: {fmt(runs)})')
    ms, runs = timed(lambda: rend(verts, background=bg, points=joints2d))
    lines.append(f'BodyRenderer, B = {B} frames, chunk {args.chunk}, background and points: {ms / B:.3f} ms per frame = {B / ms * 1e3:.0f} frames/s   '
                 f'(runs, ms: {fmt(runs)})')
    ms_d, runs_d = timed(lambda: [render_depth(verts[b], faces) for b in range(B)])
    lines.append(f'{B} calls of occlusion.render_depth on the same frames (depth only, no ids, no image): {ms_d / B:.3f} ms per frame   '
                 f'(runs, ms: {fmt(runs_d)})')
    got = rend(verts[:n], return_face_ids=True)[1]
    lines.append(f'  the body covers {float((got >= 0).float().mean()):.3f} of the image')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
