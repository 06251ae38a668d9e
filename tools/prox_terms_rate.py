"""Time per iteration of the PROX window with the optional terms: ``ProxWindowEngine.step`` against ``ProxTemporalFitter.step(use_graph=True)``.

    python tools/prox_terms_rate.py [--frames 100] [--scan 20000] [--out profiles/prox_terms_rate.txt]

Shape: ``prox_full_problem('S3')`` (B = 100 frames, V = 10475, 256^3 SDF) with 20908 faces from ``synthetic.local_faces`` over the posed
vertices of frame 0, a padded scan of S points per frame (60 .. 100 % valid, drawn from the posed vertices plus 1 cm of noise), a floor
+ box scene of ~5000 vertices against 1121 contact vertices, and the arg-max-joint segmentation of ``segmentation_from_weights``.  Rows:
no optional term, each term alone, all together.  Both sides run the same searches (``lemo_chamfer_*``, ``lemo_vertex_visibility``,
``lemo_selfpen_search``); the engine replaces the torch algebra and autograd around them by the kernels of csrc/prox_terms_kernels.hip
inside its captured iteration.

Per-iteration time = (time of step(n2) - time of step(n1)) / (n2 - n1), host clock around calls that end in a device synchronise, so
that the fitter's three eager iterations and its capture (paid inside every ``step`` call) cancel; median and spread (min .. max) of
``--runs`` repeats after one warm-up pair, engine and fitter alternating.  The synthetic sequence stretches some of frame 0's
triangles in the other frames, which inflates the collision counts against a real body mesh; the pairs per frame are printed.  There
is no earlier figure and no threshold: the file records what was measured and on which GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def scene_points():
    g = np.arange(-3.0, 3.0001, 0.1)
    fx, fy = np.meshgrid(g, g, indexing='ij')
    floor = np.stack([fx.ravel(), fy.ravel(), np.full(fx.size, 1.40)], -1)
    u = np.arange(0.0, 0.5001, 0.05)
    bx, by, bz = np.meshgrid(0.3 + u, -2.2 + u, 1.40 + u, indexing='ij')
    return np.concatenate([floor, np.stack([bx.ravel(), by.ravel(), bz.ravel()], -1)]).astype(np.float32)


def modules(prob, dev, move):
    from lemo_amd.body_model import create
    from lemo_amd.priors import Enc
    from lemo_amd.vposer import VPoser
    bm = create(prob['model'], batch_size=prob['B']).to(dev)
    vp = VPoser().eval()
    vp.load_state_dict({**vp.state_dict(), **{k: torch.from_numpy(v) for k, v in prob['vposer_w'].items()}})
    enc = Enc()
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in prob['enc_w'].items()})
    return (bm, vp.to(dev), enc.to(dev)) if move else (bm, vp, enc)


def make(cls, prob, dev, **kw):
    from lemo_amd.prox import ProxWindowEngine
    bm, vp, enc = modules(prob, dev, cls is not ProxWindowEngine)
    extra = dict(joint_map=prob['joint_map']) if cls is ProxWindowEngine else {}
    params = {k: np.array(v, copy=True) for k, v in prob['params'].items()}
    return cls(bm, vp, enc, prob['ids'], prob['Xmean'], prob['Xstd'], prob['weights'], prob['R'], prob['t'], torch.from_numpy(prob['sdf']).to(dev),
               prob['grid_min'], prob['grid_max'], params, prob['gt_joints'], prob['joints_conf'], fric_ids=prob['fric_ids'],
               first_batch_flag=False, **prob['infill'], **extra, **kw)


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--scan', type=int, default=20000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--n1', type=int, default=8)
    ap.add_argument('--n2', type=int, default=28)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'prox_terms_rate.txt'))
    a = ap.parse_args()
    import __graft_entry__ as G
    from lemo_amd import synthetic
    from lemo_amd.prox import ProxTemporalFitter, ProxWindowEngine
    from lemo_amd.selfpen import segmentation_from_weights
    dev = torch.device('cuda', 0)
    B, S = a.frames, a.scan
    prob = G.prox_full_problem('S3', B=B)
    V = prob['V']
    fit = make(ProxTemporalFitter, prob, dev)
    with torch.no_grad():
        body_pose = fit.vposer.decode(fit.pose_embedding, output_type='aa').view(B, -1)
        verts = fit.body_model(return_verts=True, body_pose=body_pose).vertices.detach().contiguous()
    faces = synthetic.local_faces(verts[0].cpu().numpy(), 20908)
    prob['model'] = dict(prob['model'], f=faces)
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    spn = torch.randint(6 * S // 10, S + 1, (B,), generator=g).to(torch.int32).to(dev)
    pick = torch.randint(0, V, (B, S), generator=g).to(dev)
    scan = torch.gather(verts, 1, pick[..., None].expand(-1, -1, 3)) + 0.01 * torch.randn(B, S, 3, generator=g).to(dev)
    scan = (scan * (torch.arange(S, device=dev)[None, :, None] < spn[:, None, None])).contiguous()
    body_mask = (torch.rand(V, generator=g) < 0.52).to(dev)
    scene = torch.from_numpy(scene_points()).to(dev)
    ids = rng.permutation(V)[:1121]
    parents = np.where(synthetic.SMPLX_PARENTS < 0, -1, synthetic.SMPLX_PARENTS)
    segm, par = segmentation_from_weights(prob['model']['weights'], faces, parents)
    terms = dict(
        none=({}, {}),
        contact=(dict(scene_v=scene, contact_verts_ids=ids), dict(contact_loss_weight=1.0)),
        scan=(dict(scan=scan, scan_point_num=spn, body_mask=body_mask), dict(s2m_weight=1.0, m2s_weight=1.0, rho_s2m=0.1, rho_m2s=0.1)),
        selfpen=(dict(faces_segm=segm, faces_parents=par, selfpen=dict(sigma=1e-4)), dict(coll_loss_weight=0.01)),
        velocity=({}, dict(smooth_vel_weight=1.0, smooth_acc_weight=1.0)))
    terms['all'] = ({k: v for kw, _ in terms.values() for k, v in kw.items()}, {k: v for _, w in terms.values() for k, v in w.items()})
    lines = [f'prox_terms_rate: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'B = {B} frames, V = {V}, F = {len(faces)}, S = {S} padded scan points with {int(spn.min())} .. {int(spn.max())} valid, scene '
             f'{scene.shape[0]} vertices, {len(ids)} contact vertices',
             f'ms per iteration = (step({a.n2}) - step({a.n1})) / {a.n2 - a.n1}: median (min .. max) of {a.runs} runs',
             f'  {"terms":<10s} {"ProxWindowEngine.step":>34s} {"ProxTemporalFitter.step(use_graph)":>40s}   fitter / engine']
    side = torch.cuda.Stream(dev)
    for name, (kw, w) in terms.items():
        p = dict(prob, weights=dict(prob['weights'], **w))
        eng, fit = make(ProxWindowEngine, p, dev, **kw), make(ProxTemporalFitter, p, dev, **kw)

        def eng_step(n):
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                eng.step(n, use_graph=True)

        rows = {'eng': [], 'fit': []}
        for r in range(a.runs + 1):
            for tag, fn in (('eng', eng_step), ('fit', lambda n: fit.step(n, use_graph=True))):
                t1, t2 = clock(lambda: fn(a.n1)), clock(lambda: fn(a.n2))
                if r:
                    rows[tag].append((t2 - t1) / (a.n2 - a.n1))
        ld = eng.loss_dict()
        note = ''
        if eng.terms is not None and 'pair_count' in eng._terms_t:
            c = eng._terms_t['pair_count']
            note = f'   pairs per frame {int(c.min())} .. {int(c.max())} (list holds {eng.terms.max_pairs})'
        e, f = rows['eng'], rows['fit']
        lines.append(f'  {name:<10s} {np.median(e):14.3f}  ({min(e):.3f} .. {max(e):.3f}) {np.median(f):20.3f}  ({min(f):.3f} .. {max(f):.3f})   '
                     f'{np.median(f) / np.median(e):6.2f} x{note}')
        lines.append(f'  {"":<10s} engine total_loss {ld["total_loss"]:.6g}, non-finite step {eng.nonfinite_step()}')
        del eng, fit
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
