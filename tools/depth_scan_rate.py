"""Time per call of depth frames -> body scans (lemo_amd/depth.py: csrc/depth_scan_kernels.hip).

    python tools/depth_scan_rate.py [--frames 100] [--out profiles/depth_scan_rate.txt]

Shape: B = 100 Kinect-like depth frames of 424 x 512 (a wavy surface around 2 m with 10 % holes), a 1080 x 1920 body mask per frame
(an ellipse of zeros), S = 20000, mask_on_color, coord = 'color': what the PROX loader does per frame.  Reported: ``create_scan`` on
float32 and on raw uint16 depth, ``unproject_depth_image`` alone, and next to them (a) the float64 numpy restatement of
projection_utils.py:35-90 + data_parser_slide.py:306-323 per frame on the CPU (host clock, 3 frames, scaled to B) and (b) a composition
of torch operations on the same device: elementwise math from the same ray table, a gather of the mask, ``nonzero`` and a per-frame
pad (it waits for the device once per frame, as ``nonzero`` must).  Device events, median and spread (min .. max) of 7 runs after 2
warm-up runs; each timed window repeats the call until it is >= 250 ms (about 2 s per row).  Next to the device-event time every row
shows the host's time to ISSUE one call (host clock around the same loop, before the synchronise): where the two are equal the row
measures the host's enqueue rate, not the device.  ``lemo_depth_scan alone`` calls the C entry point with preallocated outputs, i.e.
without the six allocations ``create_scan`` makes per call.  The same 100 frames are read in every repeat: 87 MB of depth and the part
of 207 MB of masks that the points project to stay in the 256 MB last-level cache, so nothing here is an HBM rate.  The bytes the
three passes touch are computed from the shapes; the rate over them is a whole-call figure (three launches and their gaps), not a
kernel's share of peak.  There is no earlier figure to compare with and no threshold: the file records what was measured and on
which GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from lemo_amd.depth import DepthProjection, rodrigues, undistorted_rays      # noqa: E402


def timed(fn, runs=7, warm=2, window_ms=250.0):
    """-> (median, min, max) ms per call by device events, and the median host time to issue one call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    reps = max(1, int(np.ceil(window_ms / max(a.elapsed_time(b), 1e-3))))
    out, issue = [], []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        issue.append((time.perf_counter() - t0) * 1e3 / reps)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out)), float(np.median(issue))


def calibration():
    Rd = rodrigues([0.01, -0.02, 0.005])
    dc = dict(camera_mtx=[[366.0, 0, 256.7], [0, 366.0, 206.3], [0, 0, 1]], k=[0.0925, -0.2719, 0.0005, -0.0003, 0.0927],
              view_mtx=np.hstack([Rd, [[0.002], [0.001], [-0.003]]]).tolist())
    rc, Tc = [0.003, -0.004, 0.002], [0.052, 0.0005, -0.001]
    cc = dict(camera_mtx=[[1060.5, 0, 951.3], [0, 1060.4, 536.8], [0, 0, 1]], k=[0.0519, -0.0563, 0.0008, -0.0006, 0.0134], R=rc, T=Tc,
              view_mtx=np.hstack([rodrigues(rc), np.asarray(Tc)[:, None]]).tolist())
    return dc, cc


def frames(B, H=424, W=512, cH=1080, cW=1920):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    raw = np.empty((B, H, W), np.uint16)
    Y, X = np.mgrid[0:cH, 0:cW]
    mask = np.full((B, cH, cW), 255, np.uint8)
    for b in range(B):
        d = 2.0 + 0.5 * np.sin(xx / 37.0 + 0.1 * b) + 0.3 * np.cos(yy / 23.0) + rng.normal(0, 0.01, (H, W))
        d[rng.random((H, W)) < 0.1] = 0
        raw[b] = np.round(d * 8000)
        mask[b][((X - 900 - 2 * b) / 300.0) ** 2 + ((Y - 560) / 420.0) ** 2 < 1] = 0
    return raw, mask


def numpy_frame(depth, mask, dc, cc, rays, Rc, TH=1e-2, S=20000):
    """the float64 restatement for one frame -> (scan [S, 3], count, init_trans)"""
    H, W = depth.shape
    V = np.asarray(dc['view_mtx'])
    p = (np.stack([rays[..., 0] * depth, rays[..., 1] * depth, depth], -1).reshape(-1, 3) - V[:, 3]) @ V[:, :3]
    k, M = np.asarray(cc['k']), np.asarray(cc['camera_mtx'])
    with np.errstate(all='ignore'):
        q = p @ Rc.T + np.asarray(cc['T'])
        x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        r2 = x * x + y * y
        cd = 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
        u = M[0, 0] * (x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)) + M[0, 2]
        v = M[1, 1] * (y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y) + M[1, 2]
        ui, vi = np.round(u), np.round(v)
        ok = (ui >= 0) & (ui < mask.shape[1]) & (vi >= 0) & (vi < mask.shape[0])
    keep = ok.copy()
    keep[ok] = mask[vi[ok].astype(int), ui[ok].astype(int)] == 0
    Vc = np.asarray(cc['view_mtx'])
    pc = p[keep] @ Vc[:, :3].T + Vc[:, 3]
    pc = pc[pc[:, 2] > TH]
    scan = np.zeros((S, 3), np.float32)
    scan[:min(S, len(pc))] = pc[:S]
    return scan, len(pc), pc.mean(0)


def torch_composition(depth, mask, rays, dc, cc, Rc, TH=1e-2, S=20000):
    """the same on the device in torch operations, float32: elementwise math, gather, nonzero, per-frame pad"""
    dev = depth.device
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    V, Vc, k, M = t(dc['view_mtx']), t(cc['view_mtx']), [float(v) for v in cc['k']], np.asarray(cc['camera_mtx'])
    B, H, W = depth.shape
    p = (torch.stack([rays[..., 0] * depth, rays[..., 1] * depth, depth], -1).reshape(B, -1, 3) - V[:, 3]) @ V[:, :3]
    q = p @ t(Rc).T + t(cc['T'])
    x, y = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    r2 = x * x + y * y
    cd = 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
    u = float(M[0, 0]) * (x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)) + float(M[0, 2])
    v = float(M[1, 1]) * (y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y) + float(M[1, 2])
    ui, vi = torch.round(u), torch.round(v)
    cH, cW = mask.shape[1:]
    ok = (ui >= 0) & (ui < cW) & (vi >= 0) & (vi < cH)
    flat = torch.where(ok, vi * cW + ui, torch.zeros_like(ui)).long()
    pc = p @ Vc[:, :3].T + Vc[:, 3]
    keep = ok & (torch.gather(mask.reshape(B, -1), 1, flat) == 0) & (pc[..., 2] > TH)
    scan = torch.zeros(B, S, 3, device=dev)
    trans = torch.empty(B, 3, device=dev)
    for b in range(B):
        pts = pc[b][torch.nonzero(keep[b]).flatten()]
        trans[b] = pts.mean(0)
        scan[b, :min(S, pts.shape[0])] = pts[:S]
    return scan, keep.sum(1), trans


def native_call(proj, mask, depth, S):
    """the C entry point as create_scan calls it, with every output and the workspace allocated once"""
    import ctypes as C
    from lemo_amd import _hip
    lib, dev = _hip.get_lib(), depth.device
    B, H, W = depth.shape
    cal, _ = proj._calibration(H, W)
    nbytes = int(lib.depth_scan_ws_bytes(B, H, W))
    scan = torch.empty(B, S, 3, device=dev)
    spn, nv = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    it, ws = torch.empty(B, 3, device=dev), torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    args = (depth.data_ptr(), 0, 0, 1e-3, mask.data_ptr(), 1, 1, 1e-2, C.byref(cal), B, H, W, S, scan.data_ptr(), spn.data_ptr(), nv.data_ptr(),
            it.data_ptr(), None, None, ws.data_ptr(), nbytes)
    keep = (scan, spn, nv, it, ws)

    def call(_keep=keep):
        lib.check(lib.depth_scan(*args, lib.stream(dev)), 'depth_scan')
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'depth_scan_rate.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'depth_scan_rate needs the GPU: a rate is not measured on a CPU'
    dev = torch.device('cuda', 0)
    B, H, W, cH, cW, S = a.frames, 424, 512, 1080, 1920, 20000
    dc, cc = calibration()
    raw_h, mask_h = frames(B)
    proj = DepthProjection(depth_cam=dc, color_cam=cc, color_size=(cH, cW), device=dev)
    raw, mask = torch.from_numpy(raw_h).to(dev), torch.from_numpy(mask_h).to(dev)
    depth_h = (raw_h.astype(np.float32) * np.float32(0.125)) * np.float32(1e-3)
    depth = torch.from_numpy(depth_h).to(dev)
    rays = proj.rays(H, W)
    out = proj.create_scan(mask, depth, S=S)
    out_raw = proj.create_scan(mask, raw, S=S, raw=True)
    same = all(torch.equal(out[k], out_raw[k]) for k in ('scan', 'scan_point_num', 'n_valid'))
    base = torch_composition(depth, mask, rays, dc, cc, proj.Rc)
    agree = float((base[1].int() == out['n_valid']).float().mean())
    rays64 = undistorted_rays(dc['camera_mtx'], dc['k'], H, W)
    t0 = time.perf_counter()
    cnt = [numpy_frame(depth_h[b].astype(np.float64), mask_h[b], dc, cc, rays64, proj.Rc)[1] for b in range(3)]
    cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    n = out['n_valid'].cpu().numpy()
    moved = B * (2 * H * W * (4 + 8 + 1) + 12 * S)                # passes A and C: depth, ray, one gathered mask byte; the scan
    lines = [f'depth_scan_rate: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'B = {B} frames of {H} x {W}, mask {cH} x {cW}, S = {S}, mask_on_color, coord = color; valid points per frame '
             f'{int(n.min())} .. {int(n.max())} (float64 numpy on frames 0..2: {cnt}, device: {n[:3].tolist()})',
             f'raw uint16 path == float path on every bit: {same}; frames whose count equals the torch composition\'s: {agree:.2f}',
             'ms per call by device events: median (min .. max) of 7 runs of >= 250 ms each; [host ms to issue one call]']
    res = {}

    def row(name, fn):
        res[name] = timed(fn)
        lines.append(f'  {name:<58s} {res[name][0]:9.3f}  ({res[name][1]:.3f} .. {res[name][2]:.3f})  [{res[name][3]:.3f}]')

    row('create_scan, float32 depth', lambda: proj.create_scan(mask, depth, S=S))
    row('lemo_depth_scan alone (preallocated outputs)', native_call(proj, mask, depth, S))
    row('create_scan, raw uint16 depth', lambda: proj.create_scan(mask, raw, S=S, raw=True))
    row('create_scan, float32 depth, return_pixels', lambda: proj.create_scan(mask, depth, S=S, return_pixels=True))
    row('unproject_depth_image', lambda: proj.unproject_depth_image(depth))
    row('torch composition (elementwise, gather, nonzero, pad)', lambda: torch_composition(depth, mask, rays, dc, cc, proj.Rc))
    k = 'create_scan, float32 depth'
    lines.append(f'  float64 numpy restatement on the CPU, {cpu_ms:.1f} ms per frame x {B} frames = {cpu_ms * B:.0f} ms (host clock, 3 frames)')
    lines.append(f'create_scan touches {moved / 1e6:.1f} MB per call as counted from the shapes (the 1.7 MB ray table is counted once per frame '
                 f'although every frame reads the same one from cache): {moved / res[k][0] / 1e6:.1f} GB/s over the whole call (three launches and '
                 f'their gaps; not a kernel\'s share of peak and not an HBM rate)')
    bound = 'the host (issue time = event time: the figure is the enqueue rate)' if res[k][3] >= 0.9 * res[k][0] else \
        'the device (the host issues a call faster than the device finishes one)'
    lines.append(f'create_scan at this shape is bound by {bound}: {res[k][3]:.3f} ms to issue, {res[k][0]:.3f} ms by events')
    lines.append(f'torch composition / create_scan = {res["torch composition (elementwise, gather, nonzero, pad)"][0] / res[k][0]:.1f} x; '
                 f'numpy on the CPU / create_scan = {cpu_ms * B / res[k][0]:.0f} x')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
