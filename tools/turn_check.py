"""The encoder's turn launch (csrc/conv_turn_kernels.hip) on the GPU: its error against float64 at 245 x 134 on the encoder's own layer-9
weights (tests/turn_common.py), its wall time next to the three launches it replaces in the step (layer 9 forward as a split launch,
the smoothness loss, layer 3's backward-data as a split launch: HIP events around 20 launches each), and the per-wave census of the
launch (shader-clock stamps: staging / layer 9 forward / stencil / dpre planes / layer 9 backward).  Diagnostic, GPU box only."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.assets import load_assets
from lemo_amd.priors import EncWeights, cg8p_alloc, to_cg8p
import turn_common as T

lib = _hip.get_lib(); dev = torch.device('cuda:0')
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (245, 134)
r = T.run_turn(lib, dev, H, W)
print('error vs float64 at %d x %d: z %.3e x mag (max rel %.2e), d(pre-act 9) %.3e x mag (max rel %.2e); d(pre-act 10) bit-identical to '
      'lemo_smooth_loss on the published z' % (H, W, r[0][0], r[0][1], r[1][0], r[1][1]))

enc = EncWeights(load_assets()['enc_w'], dev)
g = torch.Generator().manual_seed(0)
x = to_cg8p(T.turn_input(H, W, 1)).to(dev)
z, o, d, t2 = (cg8p_alloc(64, H, W, dev) for _ in range(4))
acc = torch.zeros(512, dtype=torch.float64, device=dev)
part = torch.zeros(lib.smooth_loss_blocks(H, W, 64), dtype=torch.float32, device=dev)
s = torch.cuda.current_stream(dev).cuda_stream
(pf, iF), (pb, iB) = enc.split_pack(9, False, 5), enc.split_pack(9, True, 5)
(p3, i3) = enc.split_pack(3, True, 5)
coef2 = 1.0 / (64 * H * (W - 1))


def turn():
    lib.check(lib.conv3x3_turn_f16(ptr(x), ptr(pf), iF, ptr(enc.b[9]), ptr(pb), iB, ptr(z), ptr(o), ptr(acc), coef2, H, W, None, None, s))


def three():
    lib.check(lib.conv3x3_mfma_split_f16(ptr(x), ptr(pf), iF, ptr(enc.w[9]), ptr(enc.b[9]), None, ptr(z), H, W, 64, 64, 0, s))
    lib.check(lib.smooth_loss(ptr(z), ptr(d), ptr(part), H, W, 64, coef2, s))
    lib.check(lib.conv3x3_mfma_split_f16(ptr(d), ptr(p3), i3, ptr(enc.wbwd[3]), None, ptr(x), ptr(t2), H, W, 64, 64, 1, s))


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


tt, t3 = timeit(turn), timeit(three)
print('turn launch back to back                                  %.2f us' % tt)
print('split<0> layer 9 + smooth loss + split<1> layer 3 (3 launches) %.2f us' % t3)

ntiles = ((W + 11) // 12) * ((H + 11) // 12)
dbg = torch.zeros(ntiles * 8 * 8, dtype=torch.int64, device=dev)
for it in range(3):
    dbg.zero_()
    lib.check(lib.conv3x3_turn_f16(ptr(x), ptr(pf), iF, ptr(enc.b[9]), ptr(pb), iB, ptr(z), ptr(o), None, coef2, H, W, None, ptr(dbg), s))
    torch.cuda.synchronize()
dd = dbg.cpu().numpy().reshape(ntiles, 8, 8)
t0, tp, tz, ts, tpl, t1 = (dd[..., k] for k in range(1, 7))
med = lambda a: int(np.median(a))
print('%d workgroups; per-wave cycles median %d max %d; staging %d | layer 9 forward + z tile %d | stencil + max %d | dpre planes %d | '
      'layer 9 backward + stores %d' % (ntiles, med(t1 - t0), (t1 - t0).max(), med(tp - t0), med(tz - tp), med(ts - tz), med(tpl - ts), med(t1 - tpl)))
wg = (t1.max(1) - t0.min(1))
print('per-workgroup lifetime median %d max %d cycles; launch span %d cycles' % (med(wg), wg.max(), t1.max() - t0.min()))
