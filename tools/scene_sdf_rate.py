"""Rate of the scene signed-distance build (lemo_amd.scene.build_scene_sdf, csrc/scene_sdf_kernels.hip).  Input: a synthetic room -- a
floor, two walls, three boxes and two free-standing sheets, tessellated at --res metres (about 2e5 triangles at the default), turned
off the lattice.  Measures GRID at 32^3 .. 256^3, BRUTE at the sizes where its predicted time stays under --limit seconds
(the prediction is the previous size x 8), and the same definition composed in torch (chunked, distance and winner only) at the sizes
where that stays under the limit.  A second table times brute force against the grid on small closed meshes at 128^3: the line where
the grid starts to win is what SDF_AUTO_FACES in the kernel file is set from.  Writes profiles/scene_sdf_rate.txt.

    python tools/scene_sdf_rate.py [--res 0.027] [--limit 10] [--out profiles/scene_sdf_rate.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def sheet(origin, u, v, res):
    origin, u, v = (np.asarray(x, np.float64) for x in (origin, u, v))
    nu, nv = max(1, int(round(np.linalg.norm(u) / res))), max(1, int(round(np.linalg.norm(v) / res)))
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    pts = origin + i.reshape(-1, 1) * u / nu + j.reshape(-1, 1) * v / nv
    a, b = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    i00, i10, i11, i01 = (a * (nv + 1) + b).ravel(), ((a + 1) * (nv + 1) + b).ravel(), ((a + 1) * (nv + 1) + b + 1).ravel(), (a * (nv + 1) + b + 1).ravel()
    return pts, np.concatenate([np.stack([i00, i10, i11], 1), np.stack([i00, i11, i01], 1)])


def box(lo, hi, res):
    """six tessellated faces, outward"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    return [sheet(lo, ey, ex, res), sheet(lo + ez, ex, ey, res), sheet(lo, ex, ez, res), sheet(lo + ey, ez, ex, res), sheet(lo, ez, ey, res),
            sheet(lo + ex, ey, ez, res)]


def room(res):
    parts = [sheet([0, 0, 0], [6, 0, 0], [0, 5, 0], res),                  # floor, normal +z
             sheet([0, 0, 0], [0, 5, 0], [0, 0, 2.6], res),                # wall x = 0, normal +x
             sheet([0, 0, 0], [0, 0, 2.6], [6, 0, 0], res)]                # wall y = 0, normal +y
    parts += box([1.0, 1.2, 0.0], [2.0, 1.8, 0.5], res) + box([3.2, 2.5, 0.0], [4.4, 3.3, 0.75], res) + box([4.8, 0.4, 0.0], [5.5, 1.4, 1.9], res)
    parts += [sheet([2.2, 3.6, 0.4], [1.5, 0.2, 0], [0, 0, 1.0], res), sheet([0.8, 3.9, 0.9], [1.0, 0, 0.1], [0, 0.8, 0], res)]
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + n); n += len(v)
    v = np.concatenate(vs) @ rot([0.1, -0.05, 1.0], 0.19).T + np.array([-2.713, -2.291, -1.137])
    return v.astype(np.float32), np.concatenate(fs)


def timed(fn, reps=5):
    """median (min) ms; a call that takes more than a second is timed once (its first run)"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    first = once()
    if first > 1000:
        return first, first
    ms = [once() for _ in range(reps + 2)][2:]
    return float(np.median(ms)), float(np.min(ms))


def torch_sdf(verts, faces_t, centres, chunk_v=4096, chunk_t=8192):
    """the definition composed in torch (float32): Ericson's regions with torch.where over [voxels, triangles] blocks -> (d^2, winner)"""
    A, B, C = (verts[faces_t[:, k]] for k in range(3))
    P = centres.reshape(-1, 3)
    best = torch.full((P.shape[0],), float('inf'), device=P.device)
    arg = torch.full((P.shape[0],), -1, dtype=torch.long, device=P.device)
    dot = lambda x, y: (x * y).sum(-1)
    for s in range(0, P.shape[0], chunk_v):
        p = P[s:s + chunk_v, None, :]
        bd = best[s:s + chunk_v].clone()
        ba = arg[s:s + chunk_v].clone()
        for t in range(0, A.shape[0], chunk_t):
            a, ab, ac = A[None, t:t + chunk_t], (B - A)[None, t:t + chunk_t], (C - A)[None, t:t + chunk_t]
            ap = p - a
            bp, cp = ap - ab, ap - ac
            d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            e43, e56 = d4 - d3, d5 - d6
            one, zero = torch.ones_like(d1), torch.zeros_like(d1)
            ns, nt, dn = vb, vc, va + vb + vc
            for cond, s_, t_, n_ in (((va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                     ((d6 >= 0) & (d5 <= d6), zero, one, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                     ((d3 >= 0) & (d4 <= d3), one, zero, one), ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
                ns, nt, dn = torch.where(cond, s_, ns), torch.where(cond, t_, nt), torch.where(cond, n_, dn)
            q = ap - (ns / dn)[..., None] * ab - (nt / dn)[..., None] * ac
            dd = dot(q, q)
            m, i = dd.min(dim=1)
            upd = m < bd
            bd, ba = torch.where(upd, m, bd), torch.where(upd, i + t, ba)
        best[s:s + chunk_v], arg[s:s + chunk_v] = bd, ba
    return best, arg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=float, default=0.027)
    ap.add_argument('--limit', type=float, default=10.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_sdf_rate.txt'))
    a = ap.parse_args()
    from lemo_amd.scene import build_scene_sdf, prepare_scene_mesh
    device = torch.device('cuda', 0)
    v, f = room(a.res)
    mesh = prepare_scene_mesh(torch.from_numpy(v).to(device), f)
    gmin, gmax = mesh.box_min - 0.25, mesh.box_max + 0.25
    lines = [f'scene SDF build, synthetic room: V = {len(v)}, F = {len(f)}, box {np.round(gmax - gmin, 3).tolist()} m; {torch.cuda.get_device_name(0)}; '
             f'median (min) ms of the native call (tables prepared once, not timed)']
    kw = dict(grid_min=gmin, grid_max=gmax)
    brute_pred, torch_pred, ref = 0.0, 0.0, {}
    for dim in (32, 64, 128, 256):
        run = lambda **k: build_scene_sdf(mesh, dim=dim, **kw, **k)
        row = [f'{dim:3d}^3']
        S = run(mode='grid', return_nearest=True)
        for g in (None, 16, 32):
            med, mn = timed(lambda: run(mode='grid', grid=g))
            row.append(f'grid {"default" if g is None else g} {med:9.3f} ({mn:.3f})')
        if brute_pred * 8 <= a.limit * 1000:
            Sb = run(mode='brute', return_nearest=True)
            assert torch.equal(Sb.sdf.view(torch.int32), S.sdf.view(torch.int32)) and torch.equal(Sb.nearest, S.nearest), f'grid != brute at {dim}'
            med, mn = timed(lambda: run(mode='brute'), reps=3)
            brute_pred = med
            row.append(f'brute {med:10.3f} ({mn:.3f}) [bit-identical to grid]')
        else:
            row.append(f'brute skipped (predicted {brute_pred * 8 / 1000:.0f} s > {a.limit:.0f} s)')
        if torch_pred * 8 <= a.limit * 1000:
            ft = mesh.faces.long()
            out = []
            med, mn = timed(lambda: out.append(torch_sdf(mesh.vertices, ft, S.centres())), reps=1)
            err = float((out[0][0].sqrt() - S.sdf.abs().reshape(-1)).abs().max())
            torch_pred = med
            row.append(f'torch {med:10.3f} ({mn:.3f}) [max |d - d_torch| {err:.2e}]')
        else:
            row.append(f'torch skipped (predicted {torch_pred * 8 / 1000:.0f} s > {a.limit:.0f} s)')
        lines.append('  '.join(row))
        if dim == 256:
            lines.append(f'256^3: {float((S.sdf < 0).float().mean()) * 100:.1f} % of the voxels negative')

    lines.append('')
    lines.append('small meshes at 128^3 (a 1.0 x 0.8 x 1.2 m box, each face cut into n x n x 2 triangles): brute force against the grid, median (min) ms '
                 '-- what SDF_AUTO_FACES is set from')
    for n in (1, 2, 3, 4, 6, 8, 16, 32):
        vs, fs, k = [], [], 0
        for pv, pf in box([-0.5, -0.4, -0.6], [0.5, 0.4, 0.6], 1.0 / n):
            vs.append(pv); fs.append(pf + k); k += len(pv)
        sv, sf, name = np.concatenate(vs) @ rot([0.3, 1.0, 0.2], 0.37).T + np.array([0.113, -0.047, 1.021]), np.concatenate(fs), f'box n = {n}'
        m = prepare_scene_mesh(torch.from_numpy(sv.astype(np.float32)).to(device), sf)
        k2 = dict(dim=128, grid_min=m.box_min - 0.25, grid_max=m.box_max + 0.25)
        b = timed(lambda: build_scene_sdf(m, mode='brute', **k2))
        g = timed(lambda: build_scene_sdf(m, mode='grid', **k2))
        lines.append(f'{name:13s} F = {len(sf):5d}  brute {b[0]:8.3f} ({b[1]:.3f})  grid {g[0]:8.3f} ({g[1]:.3f})')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
