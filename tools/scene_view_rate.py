"""Time per frame of ``SceneView`` (lemo_amd/scene_view.py), pass by pass, next to what the pieces of the library before it could be
composed into: ``BodyRenderer`` with ``return_depth``, one ``render_depth`` of the scene, and ``torch.where``.

    python tools/scene_view_rate.py [--frames 100] [--chunk 16] [--out profiles/scene_view_rate.txt]

The scene is a synthetic room of about 2 * 10^5 coloured triangles (a wavy floor, 316 x 316 cells), the body the SMPL-X-shaped
synthetic model (V = 10475, F = 20908, faces redrawn as small triangles, ``synthetic.local_faces``) in ``--frames`` poses, seen from
2.7 m so that floor, body and background all show; 81 spheres of 2 cm float in front of the marker vertices; 1920 x 1080.  The passes are timed
through the C entry points on ``--chunk`` frames at a time, the whole call through ``SceneView``.  Device events around the repeated
launches, median of 5 runs after one warm-up.  No rate is asserted anywhere: the file records what was measured and on which GPU.
NOTHING OF THIS WAS MEASURED BEFORE SceneView EXISTED: there was no device path for these views to time.
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
from lemo_amd.assets import load_vertex_ids                      # noqa: E402
from lemo_amd.body_model import create                           # noqa: E402
from lemo_amd.occlusion import PROX_RENDER, render_depth         # noqa: E402
from lemo_amd.render import BodyRenderer                         # noqa: E402
from lemo_amd.scene_view import SceneView                        # noqa: E402


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


def room(cells=316):
    """a wavy floor 1 m below the camera, cells x cells quads, in camera coordinates, with checker-board vertex colours"""
    gx, gz = np.meshgrid(np.linspace(-3, 3, cells + 1), np.linspace(0.6, 9, cells + 1), indexing='ij')
    v = np.stack([gx, 1.0 + 0.02 * np.sin(3 * gx) * np.cos(2 * gz), gz], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int32)
    ii, jj = np.divmod(np.arange(len(v)), cells + 1)
    col = np.stack([60 + 150 * ((ii // 8 + jj // 8) % 2), 90 + (ii * 3) % 120, 200 - (jj * 2) % 150], -1).astype(np.uint8)
    return v, f, col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--chunk', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'scene_view_rate.txt'))
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
    ids = torch.from_numpy(np.asarray(load_vertex_ids()['markers81'], np.int64)).to(dev)
    P = ids.shape[0]
    # the synthetic model's marker vertices lie inside its vertex cloud: the spheres keep their x and y and float in four layers in front of it
    front = verts[..., 2].min() - 0.05 * (1 + torch.arange(P, device=dev) % 4)
    spheres = torch.cat([verts[:, ids, :2], front[None, :, None].expand(B, P, 1)], -1).contiguous()
    cols = torch.tensor([(218, 165, 32) if i % 2 else (70, 130, 180) for i in range(P)], dtype=torch.uint8, device=dev)
    radius = torch.full((P,), 0.02, device=dev)
    sv, sf, sc = room()
    back = np.eye(4); back[2, 3] = 1.4                           # the camera 1.4 m further back: the body at 2.7 m
    view = SceneView(bm.faces, scene_vertices=sv, scene_faces=sf, scene_colors=sc, view=back, chunk=args.chunk)
    V, Vs, Fs = verts.shape[1], len(sv), len(sf)
    faces = view.topology.on(dev, V)[0]
    F = faces.shape[0]
    keys = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    kid = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    normals = torch.empty(n, V, 3, device=dev)
    moved = torch.empty(n, V, 3, device=dev)
    img = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    s = lib.stream(dev)
    cam, shade, xf = C.byref(view._cam), C.byref(view._shade), view._view_xf
    _, start, face, nnz = view.topology.on(dev, V)
    v = verts[:n]
    compose = lambda sph, p: lib.check(lib.view_compose(ptr(moved), ptr(normals), n, V, ptr(faces), F, cam, ptr(keys), ptr(kid), shade, ptr(view.scene_key),
                                                        ptr(view.scene_rgb), sph, p, ptr(radius), ptr(cols), 1, xf, 0xFFFFFF, ptr(img), None, None, s))
    passes = [
        ('view_transform of the bodies', lambda: lib.check(lib.view_transform(ptr(v), n * V, xf, ptr(moved), s))),
        ('vertex normals', lambda: lib.check(lib.vertex_normals(ptr(moved), n, V, ptr(faces), F, ptr(start), ptr(face), nnz, ptr(normals), None, s))),
        ('the walk (depth pass + id pass)', lambda: lib.check(lib.render_ids(ptr(moved), n, V, ptr(faces), F, cam, ptr(keys), ptr(kid), None, s))),
        (f'compose with {P} spheres', lambda: compose(ptr(spheres[:n]), P)),
        ('compose without spheres', lambda: compose(None, 0)),
    ]
    fmt = lambda rs: ', '.join(f'{x:.2f}' for x in rs)
    lines = [f'{torch.cuda.get_device_name(0)}; {W} x {H}, body V = {V}, F = {F}; scene Vs = {Vs}, Fs = {Fs}; {P} spheres; median of 5 runs after one '
             f'warm-up (device events).  Nothing of this was measured before SceneView existed.']
    ms, runs = timed(lambda: view.set_view(back))
    lines.append(f'static layer (set_view: transform, normals, walk, resolve of the scene), once per view: {ms:.3f} ms   (runs, ms: {fmt(runs)})')
    lines.append(f'passes on {n} frames per set of launches:')
    for what, fn in passes:
        ms, runs = timed(fn)
        lines.append(f'  {what}: {ms / n:.3f} ms per frame   (runs of {n} frames, ms: {fmt(runs)})')
    kw = dict(spheres=spheres, sphere_radius=radius, sphere_colors=cols)
    ms, runs = timed(lambda: view(verts, **kw))
    lines.append(f'SceneView, B = {B} frames, chunk {args.chunk}, scene, body and {P} spheres: {ms / B:.3f} ms per frame = {B / ms * 1e3:.0f} frames/s   '
                 f'(runs, ms: {fmt(runs)})')
    ms, runs = timed(lambda: view(verts))
    lines.append(f'SceneView, the same without spheres: {ms / B:.3f} ms per frame = {B / ms * 1e3:.0f} frames/s   (runs, ms: {fmt(runs)})')
    own = view(verts[:n], spheres=spheres[:n], sphere_radius=radius, sphere_colors=cols, return_owner=True)[1]
    share = [float((own == k).float().mean()) for k in (-1, 0, 1)]
    lines.append(f'  of the image: background {share[0]:.3f}, scene {share[1]:.3f}, body {share[2]:.3f}, spheres {float((own >= 2).float().mean()):.4f}')

    # what could be composed before: the body over its own depth, the scene's depth once, torch.where per chunk; no scene colours
    # (nothing interpolated them), no spheres, the body in camera coordinates already
    rend = BodyRenderer(bm.faces, cull_backface=False, chunk=args.chunk)
    cam_verts = verts + torch.tensor([0.0, 0.0, 1.4], device=dev)
    svd, sfd = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    flat = torch.tensor([120, 130, 140], dtype=torch.uint8, device=dev)
    white = torch.full((3,), 255, dtype=torch.uint8, device=dev)

    def before():
        d_scene = render_depth(svd, sfd, back, cull_backface=False)
        res = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        for lo in range(0, B, args.chunk):
            im, d = rend(cam_verts[lo:lo + args.chunk], return_depth=True)
            body = (d != 0) & ((d_scene == 0) | (d <= d_scene))
            res[lo:lo + args.chunk] = torch.where(body[..., None], im, torch.where((d_scene != 0)[None, ..., None], flat, white))
        return res
    ms, runs = timed(before)
    lines.append(f'BodyRenderer(return_depth) + one render_depth of the scene + torch.where, B = {B}, chunk {args.chunk} (flat scene colour, no spheres): '
                 f'{ms / B:.3f} ms per frame = {B / ms * 1e3:.0f} frames/s   (runs, ms: {fmt(runs)})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
