"""The iteration kernels that have no C entry point of their own, one loss term at a time, against the float64 oracles
(tests/test_iter_terms_emu.py on the host-emulated build, tests/test_iter_terms_gpu.py on the MI355X; both run the cases below):

  prox_frame_dense, prox_sparse, prox_adam / prox_tail                 csrc/prox_kernels.hip     through lemo_amd.prox.ProxWindowEngine
  fit_losses, dverts_assemble / the fused dverts_vertex, fit_tail      csrc/loss_kernels.hip     through lemo_amd.fitting.AmassTemporalFitter

Why one term at a time.  The whole-iteration parity tests gate a gradient at 2e-4 (PROX) / 1e-3 (AMASS) of the LARGEST entry of the tensor
with every term on.  The smoothness prior owns that entry (PROX S3: max |g| 1.08e3 against 46 for the 2-D joints, 1.6 .. 0.1 for SDF
penetration, infill and friction, 1.7e-3 .. 2.9e-9 for the priors), so a prior gradient that is missing, or an infill gradient that is
50 % too large, passes.  With one weight of ``lemo_amd.prox.WEIGHT_ORDER`` (``fitting.LOSS_WEIGHTS``) non-zero the term's own gradient is
the largest entry and the same break is an error of 1.0 / 0.5.

Gate
----
For each optimised tensor ("group": the nine of ``prox.ENGINE_PARAMS``, or transl / rot6d / other)

    err_group(g) = max |g - g64| / max |g64|

against the gradient g64 of the float64 oracle at the same float32 state (``oracle.f64.prox_fit_oracle_f64`` / ``amass_fit_oracle_f64`` /
``perframe_iteration_f64``).  The yardstick of a case is the LARGEST err_group of the float32 CPU oracle (``__graft_entry__.prox_oracle_for``
/ ``oracle_for`` / ``pipeline_oracle.perframe_iteration``) over the groups of that case, and every group of the kernel must stay within
GATE = 4 yardsticks (the project's gate: ``blocks_common.GATE``).  The largest group is taken so that one group on which the float32 oracle
happens to round well does not set the bar (``lbs_common`` met a restatement at 0.14 ulp).  Where the float32 oracle's error is exactly
zero the kernel gets FLOOR = 2^-23, one ulp of the group's largest entry, as in ``blocks_common``.  A group whose float64 gradient is
identically zero (every group but ``pose_embedding`` under the body-pose prior, say) must be exactly zero from the kernel: a product with a
zero weight has no rounding.  Nothing here is fitted to what the kernels give; the kernel / yardstick ratios are collected in RATIOS and
printed by the last test of either module (DESIGN.md quotes them).

Loss entries: the entry of the term under test and ``total_loss`` within 1e-5 relative of float64 (the bound of the whole-iteration tests,
without their absolute 1e-12, which would be 5e-5 of the hand prior's 2e-8); every other entry exactly 0.0.

The three L2 priors of the AMASS fit are added inside ``fit_tail_kernel`` and never reach ``grads()``; ``grads_with_priors()`` restates them
on the host.  The kernel's own value is read from Adam's first moment: after one step from zero state ``exp_avg = 0.1f * g`` in ONE float32
product (torch's lerp from 0 with weight float(1 - 0.9); ``common.hpp adam_update_torch``), so ``exp_avg / 0.1f``, divided in float64, is
the kernel's gradient to 2^-24 relative.  Those cases get 2^-23 added to the gate: 2^-24 for that product and as much for the entry being
normalised by the group's maximum, not by itself.

Preconditions of a case (checked on the CPU BEFORE the engine runs)
-------------------------------------------------------------------
``sdf < 0``, ``sdf < 0.01``, ``|v_t| > 1e-4``, ``v_z < 0``, ``residual > 0``, ``speed > 0.1`` and the sign of the L1 residuals (2-D joints,
markers, infill) change a mean or a gradient by a JUMP when one element changes sides.  No rounding gate may absorb that, so every case must
keep every selecting quantity of its live terms, evaluated in float64, away from its threshold by more than float32 can move it; a case
that does not FAILS (it is never skipped and no element is masked out: the share of cases left out is zero).  With u = 2^-24:

  position        M_POS = 10 u 8 m = 4.8e-6 m: a vertex coordinate is the end of about ten float32 operations on numbers below 8 m (blend sum,
                  four skinning products and their sum, translation, the products and additions of cam -> world; every case asserts
                  max |coordinate| < 8 m).  That count does not hold where the seeded VPoser decoder is ill-conditioned: its Gram-Schmidt
                  step magnifies the rounding of the out layer by 1 / sin(a1, a2), and the float32 oracle itself sits 1.2e-6 .. 1.7e-5 m
                  from float64, depending on the frame and on the order in which it sums.  So the margin of frame b is
                  m_pos[b] = max(M_POS, GATE x the float32 oracle's largest position error in frame b) over 1 + N_POS_ORDERS = 9 summation
                  orders of the oracle (the 2 x 512 hidden units of the decoder renumbered: the same function) -- what the gate allows a
                  correct float32 implementation, measured on the reference and not on the code under test.
  L1 residual     marker / infill: target (an input) minus a position: m_pos[b].
  v_z, |v_t|      differences of the positions of frames b and b + 1: m_pos[b] + m_pos[b + 1] per component; the tangential norm of two
                  components: sqrt(2) times that.
  speed           30 x the norm of a three-component difference: 30 sqrt(3) (m_pos[b] + m_pos[b + 1]).
  SDF value       G m_pos[b] + (15 n + 24) u D: G = the largest |difference of neighbouring voxels| / voxel size (how far a position error
                  moves the value), n = the grid size and D = the largest difference of neighbouring voxels: each voxel coordinate is five
                  float32 operations on numbers <= n (5 u n of a voxel, each worth <= D, three axes) and the seven interpolations add
                  24 u D (``blocks_common``'s sdf_sample bound with the local D in place of 2 max |sdf|).
  2-D residual    p = f x / z + c: (f / z) (1 + max(|x|, |y|) / z) m_pos[b] for the joint's position error + 3 u |p| for the division, the
                  product and the sum.

The static window: frames with bit-identical parameters have velocity exactly 0 in the engine (the same code on the same numbers), and 0 is
on the not-selected side of all three velocity tests.  The oracles' batched products leave +-2e-16 (float64) / +-1e-7 (float32) there, so
in that case alone both oracles test ``v_z < -1e-9`` (``ProxFitOracle.thresholds``), and a pair of identical frames with |v_z| < 1e-9 is
exempt from the v_z margin.  The engine's friction and contact entries must then be exactly 0.0.

Two more preconditions keep luck out of the yardstick.  The yardstick is ONE float32 evaluation, and on a frame whose decode is
ill-conditioned single roundings decide how far it lands from float64: prox_small_problem(B=10) decodes a joint with |sin(a1, a2)| = 0.048
in frame 4; six summation orders of the float32 oracle put that frame's pose_embedding gradient 1.1e-6 .. 9.0e-6 from float64 under the
infill term (the unpermuted one is the luckiest), the engine sits at 9.7e-6 with an out-layer error equal to the oracle's (3.1 u), and with
all terms on it measured 5.3 yardsticks.  That is a property of the input, not of either implementation, so such inputs are moved like
those that sit on a threshold:
  * the largest position error of the 9 summation orders above within GATE of one another, and
  * the largest err_group of 1 + N_ORDERS = 4 of them (full closures) within GATE of one another -- the gate claims that two correct float32
    evaluations lie within a factor 4 of each other's distance from float64; a case in which the oracle's own reorderings do not, cannot test that.
The yardstick itself stays the unpermuted oracle's, as everywhere else in the suite.

Moved cases: every case runs seed 5 of ``prox_small_problem`` / ``small_problem`` and their own synthetic sequence (4 / 3) unless CASE_MOVES names
another model seed and sequence; an entry there says which precondition the default broke.  The case was moved, never the margin.  torch's
float32 CPU kernels sum in another order on another processor, so the float32 preconditions are machine-dependent: the listed instances hold on
both hosts the suite runs on (the CPU-only one and the MI355X machine's).

Cases
-----
PROX terms   ``prox_small_problem(stage='S3')`` (B = 14, V = 640), ``first_batch_flag=True``, joint weights kept, one weight on: data,
             body_pose + bending (bending follows body_pose: one case), hand, expr, jaw, SDF penetration, smoothness, friction normal /
             tangent, infill rec / contact; ``shape_weight`` has no gradient: its case checks total_loss and that every gradient is 0.
PROX edges   all terms on, ``first_batch_flag=False``: B = 10 (the smallest accepted, erase_n = 1), 13, 33 (more frames than the 32
             accumulator slots) and 41 (erase_n = 6) -- erased rows exactly 0, and after ``step(1)`` bit-equal to the input while row
             erase_n has moved; empty selections (SDF + 10, no contact label, a static window, SDF weight 0, an all-ones marker mask),
             whose count-normalised entries must be exactly 0.0; 300 friction vertices (n_s > 256: a second blockIdx.y in
             prox_sparse_kernel); and the refusals of lemo_prox_create (B = 9; use_infill with T > B - 1).
AMASS terms  ``small_problem()``: rec_markers, contact_vel, smooth with ``full_vertices`` False (fused dverts_vertex) and True;
             ``small_problem(B=12, V=1300, foot=262)`` with the three terms on for the dverts_assemble fallback (n > 1024).
AMASS priors vposer, shape (no gradient: exp_avg exactly 0), hand through ``exp_avg`` as above, and vposer + hand once more with
             ``per_frame=True`` at B = 3, where the denominators use Bn = 1."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from lemo_amd import _hip
from lemo_amd.fitting import LOSS_WEIGHTS, AmassTemporalFitter
from lemo_amd.prox import ENGINE_PARAMS, LOSS_KEYS, S3_WEIGHTS, WEIGHT_ORDER
from oracle import pipeline_oracle as PLO
from oracle.f64 import amass_fit_oracle_f64, default_f64, perframe_iteration_f64, prox_fit_oracle_f64

GATE = 4.0
FLOOR = 2.0 ** -23
U = 2.0 ** -24
LOSS_TOL = 1e-5
P_MAX = 8.0                       # metres: the docstring's bound on a coordinate; every case asserts it stays below
M_POS = 10 * U * P_MAX            # 4.8e-6 m
N_ORDERS = 3                      # further summation orders of the float32 oracle (hidden units of the decoder permuted): gradients
N_POS_ORDERS = 8                  # ... and, forward only, positions

RATIOS = {}                       # case -> (worst kernel err_group / yardstick, worst kernel err_group, yardstick)

# case -> dict(seed=model seed, seq=sequence id) where the defaults (seed 5; sequence 4 for PROX, 3 for AMASS) break a precondition.  The
# first instance of the list seq = 4, 5, 6, ... x seed = 5, 6, 7 that meets every precondition with the float32 oracle of BOTH hosts the suite
# runs on (torch's float32 CPU kernels sum in another order on the GPU machine's processor); the comment names what the default broke.
CASE_MOVES = {
    'sdf_penetration': dict(seed=7, seq=4),      # sdf < 0: two vertices inside the margin
    'B10': dict(seed=6, seq=5),                  # positions of frame 4 from 1.4e-6 to 6.7e-6 m over the summation orders (|sin(a1, a2)| = 0.048)
    'B13': dict(seed=7, seq=4),                  # sdf < 0
    'B33': dict(seed=7, seq=6),                  # sdf < 0
    'B41': dict(seed=5, seq=20),                 # sdf < 0 (five vertices); of 108 instances tried, two meet every precondition on both hosts
    'no_contact_label': dict(seed=7, seq=4),     # sdf < 0
    'static_window': dict(seed=5, seq=6),        # the oracle's own summation orders 2.4e-5 .. 0.27 apart
    'mask_all_ones': dict(seed=7, seq=4),        # sdf < 0
    'fric300': dict(seed=5, seq=6),              # sdf < 0, friction sdf < 0.01
    'smooth full=0': dict(seed=5, seq=4),        # the oracle's own summation orders 1.9e-6 .. 1.2e-5 apart
    'smooth full=1': dict(seed=5, seq=4),
}

PROX_GROUPS = tuple(n for n, _ in ENGINE_PARAMS)
AMASS_GROUPS = ('transl', 'rot6d', 'other')

# case -> (the weights switched on, the loss_dict entry that carries the term or None where only total_loss does)
PROX_TERMS = {
    'data': (('data_weight',), 'joint_loss'),
    'body_pose_bending': (('body_pose_weight',), None),
    'shape': (('shape_weight',), None),
    'hand_prior': (('hand_prior_weight',), None),
    'expr_prior': (('expr_prior_weight',), None),
    'jaw_prior': (('jaw_prior_weight',), None),
    'sdf_penetration': (('sdf_penetration_weight',), 'sdf_penetration_loss'),
    'motion_prior_smooth': (('motion_prior_smooth_weight',), 'motion_prior_smooth_loss'),
    'friction_normal': (('friction_normal_weight',), 'loss_fric_normal'),
    'friction_tangent': (('friction_tangent_weight',), 'loss_fric_tangent'),
    'motion_infill_rec': (('motion_infill_rec_weight',), 'motion_infill_loss'),
    'motion_infill_contact': (('motion_infill_contact_weight',), 'motion_infill_contact_loss'),
}
SHAPE_WEIGHT = 0.03               # S3 carries shape_weight 0; any non-zero value shows the entry (betas are not optimised)
PROX_B_SWEEP = (10, 13, 33, 41)
PROX_EMPTY = ('sdf_plus_10', 'no_contact_label', 'static_window', 'sdf_weight_0', 'mask_all_ones')
AMASS_TERMS = ('rec_markers', 'contact_vel', 'smooth')
AMASS_PRIORS = ('vposer', 'shape', 'hand')


def _f(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def err_of(v, ref):
    return float((v.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def largest_err(g, ref):
    live = [n for n in ref if float(ref[n].abs().max()) > 0]
    return max(err_of(g[n], ref[n]) for n in live) if live else 0.0


def permuted_decoder(vw, k):
    """the same VPoser decoder with its 2 x 512 hidden units renumbered: the same function, another float32 summation order"""
    rng = np.random.default_rng(100 + k)
    p1, p2 = rng.permutation(512), rng.permutation(512)
    w = dict(vw)
    w['bodyprior_dec_fc1.weight'], w['bodyprior_dec_fc1.bias'] = vw['bodyprior_dec_fc1.weight'][p1].copy(), vw['bodyprior_dec_fc1.bias'][p1].copy()
    w['bodyprior_dec_fc2.weight'], w['bodyprior_dec_fc2.bias'] = vw['bodyprior_dec_fc2.weight'][p2][:, p1].copy(), vw['bodyprior_dec_fc2.bias'][p2].copy()
    w['bodyprior_dec_out.weight'] = vw['bodyprior_dec_out.weight'][:, p2].copy()
    return w


def yardstick_is_no_luck(case, e32, others):
    """the float32 oracle under N_ORDERS other summation orders: their largest err_group within GATE of one another (module docstring)"""
    es = [max(e, FLOOR) for e in [e32] + list(others)]
    print(f'{case}: float32 oracle, largest err_group under {len(es)} summation orders: ' + ' '.join(f'{e:.3e}' for e in es))
    assert max(es) <= GATE * min(es), (f'{case}: equally valid float32 evaluations of the oracle lie {min(es):.3e} .. {max(es):.3e} from float64, more than the '
                                       f'gate\'s factor {GATE:g} apart: the case is ill-conditioned and its yardstick a matter of luck -- move the case (CASE_MOVES)')


def gate_groups(case, got, f32, ref, extra=0.0):
    """every group of the kernel within GATE x the float32 oracle's LARGEST err_group (+ `extra`); identically-zero groups exactly zero"""
    live = [n for n in ref if float(ref[n].abs().max()) > 0]
    for n in ref:
        g = got[n].detach().cpu()
        assert g.shape == ref[n].shape, (case, n)
        if n not in live:
            assert float(g.abs().max()) == 0.0, f'{case} {n}: the float64 gradient is identically zero, the kernel gives {float(g.abs().max()):.3e}'
    if not live:
        return
    e32 = max(err_of(f32[n], ref[n]) for n in live)
    bound = (GATE * e32 if e32 > 0 else FLOOR) + extra
    worst = 0.0
    for n in live:
        g = got[n].detach().cpu()
        assert torch.isfinite(g).all(), (case, n)
        e = err_of(g, ref[n])
        worst = max(worst, e)
        print(f'{case} {n}: kernel {e:.3e} float32 oracle {err_of(f32[n], ref[n]):.3e} (largest group {e32:.3e})')
    ratio = worst / e32 if e32 > 0 else 0.0
    RATIOS[case] = (ratio, worst, e32)
    for n in live:
        e = err_of(got[n].detach().cpu(), ref[n])
        assert e <= bound, (f'{case} {n}: {e:.3e} of the group\'s largest float64 entry, the float32 oracle\'s largest group {e32:.3e} '
                            f'(gate {GATE:g} x, floor {FLOOR:.1e} at zero, + {extra:.1e})')


def report_ratios():
    for k in sorted(RATIOS):
        r, e, y = RATIOS[k]
        print(f'iter_terms ratio {k}: worst kernel / float32 oracle {r:.2f}, worst kernel err_group {e:.3e}, yardstick {y:.3e}')
    assert RATIOS, 'no case ran before the report'


def _rel_close(a, b, what):
    assert math.isfinite(a) and abs(a - b) <= LOSS_TOL * abs(b), f'{what}: {a!r} against float64 {b!r}'


def _lib_arg(lib):
    return lib if lib.is_emu else None


# ---------------------------------------------------------------------------------------------------------------------------
# the selections, in float64

def _away(what, dist, margin, exempt=None):
    """every element of `dist` (distance of a selecting quantity from its threshold) beyond its `margin` (a number or a tensor like `dist`)"""
    if dist.numel() == 0:
        return
    margin = torch.as_tensor(margin, dtype=dist.dtype).expand_as(dist)
    bad = dist <= margin
    if exempt is not None:
        bad = bad & ~exempt
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} element(s) inside the margin (closest {float(dist[bad].min()):.3e}, margin there '
                                 f'{float(margin[bad][dist[bad].argmin()]):.2e}): float32 may take the other side -- move the case (CASE_MOVES), not the margin')


def position_margins(case, v32s, v64):
    """[B] position margin of every frame from the float32 oracle's own vertices under the 1 + N_POS_ORDERS summation orders (module
    docstring), after holding the orders' largest errors within GATE of one another"""
    e = torch.stack([(v.detach().double() - v64.detach()).abs().amax((1, 2)) for v in v32s])        # [orders, B]
    worst = e.amax(1)
    print(f'{case}: float32 oracle positions, largest error under {len(v32s)} summation orders (1e-6 m): ' + ' '.join(f'{float(x) * 1e6:.1f}' for x in worst))
    assert float(worst.max()) <= GATE * float(worst.min()), (
        f'{case}: equally valid float32 evaluations of the oracle place a vertex {float(worst.min()):.3e} .. {float(worst.max()):.3e} m from float64, more than '
        f'the gate\'s factor {GATE:g} apart: a frame decodes an ill-conditioned pose and single roundings decide its error -- move the case (CASE_MOVES)')
    return torch.clamp(GATE * e.amax(0), min=M_POS)


def prox_margins(case, of, m_pos, prob):
    """`of`: the float64 ProxFitOracle of the case, `m_pos` [B] its position margins.  Restates the selecting quantities of oracle/prox_oracle.py
    (:130-189) and holds each live one away from its threshold (module docstring)."""
    from oracle.prox_oracle import THRESHOLDS
    w, thr = of.w, getattr(of, 'thresholds', None) or THRESHOLDS
    with default_f64(), torch.no_grad():
        verts, joints118, _ = of._body(True)
        vw = torch.matmul(of.R, verts.permute(0, 2, 1)).permute(0, 2, 1) + of.t
        B, nv = vw.shape[0], vw.shape[1]
        P = max(float(verts.abs().max()), float(vw.abs().max()), float(joints118.abs().max()))
        assert P < P_MAX, (case, P)
        m_pair = m_pos[:-1] + m_pos[1:]                  # a difference of the positions of frames b and b + 1, per component
        pr = prob['params']
        same_next = torch.tensor([all(np.array_equal(np.asarray(pr[k])[b], np.asarray(pr[k])[b + 1]) for k in pr) for b in range(B - 1)])
        if w['data_weight'] > 0:
            proj = of.camera(joints118)
            live = ((of.joint_weights * of.joints_conf) > 0).unsqueeze(-1).expand_as(proj)
            x, y, z = joints118[..., 0], joints118[..., 1], joints118[..., 2]
            assert float(z.min()) > 0.5, (case, float(z.min()))
            f = max(of.cam['fx'], of.cam['fy'])
            m_px = f / z * (1 + torch.maximum(x.abs(), y.abs()) / z) * m_pos[:, None] + 3 * U * proj.abs().amax(-1)          # [B, 118]
            _away(f'{case}: 2-D joint residual', (of.gt_joints - proj)[live].abs(), m_px.unsqueeze(-1).expand_as(proj)[live])
        sdf = of.sdf
        n = max(sdf.shape)
        vox = ((of.grid_max - of.grid_min) / torch.tensor(sdf.shape, dtype=torch.float64))
        diffs = [(sdf.diff(dim=a).abs().max()) for a in range(3)]
        D = float(max(diffs))
        G = float(max(d / vox[a] for a, d in enumerate(diffs)))
        m_sdf = (G * m_pos + (15 * n + 24) * U * D)[:, None].expand(B, nv)
        norm_v = (vw - of.grid_min) / (of.grid_max - of.grid_min) * 2 - 1
        body_sdf = F.grid_sample(sdf[None, None].expand(B, -1, -1, -1, -1), norm_v[:, :, [2, 1, 0]].view(-1, nv, 1, 1, 3),
                                 padding_mode='border', align_corners=False).view(B, nv)
        if w['sdf_penetration_weight'] > 0:
            _away(f'{case}: sdf < 0', body_sdf.abs(), m_sdf)
        if w['friction_normal_weight'] > 0 or w['friction_tangent_weight'] > 0:
            vf = vw[:, of.fric_ids, :]
            vel = vf[1:] - vf[:-1]
            sdf_f = body_sdf[0:-1][:, of.fric_ids]
            _away(f'{case}: friction sdf < {thr["fric_sdf"]}', (sdf_f - thr['fric_sdf']).abs(), m_sdf[0:-1][:, of.fric_ids])
            sel = sdf_f < thr['fric_sdf']
            static = same_next[:, None].expand_as(sel)[sel]
            mp = m_pair[:, None].expand_as(sel)[sel]
            vc = vel[sel]
            if w['friction_tangent_weight'] > 0:
                gt_ = torch.norm(vc[:, :2], dim=-1)
                _away(f'{case}: |v_t| > {thr["fric_vt"]}', (gt_ - thr['fric_vt']).abs(), math.sqrt(2) * mp)
            if w['friction_normal_weight'] > 0:
                _away(f'{case}: v_z < 0', (vc[:, 2] - thr['fric_vn']).abs(), mp, exempt=static & (vc[:, 2].abs() < 1e-9))
        if of.body_markers_rec is not None and of.marker_mask.numel() > float(of.marker_mask.sum()):
            T = of.body_markers_rec.shape[0]
            if w['motion_infill_rec_weight'] > 0:
                markers = vw[:, of.ids['markers67'], :]
                occluded = ((1 - of.marker_mask[0:T]) > 0).unsqueeze(-1).expand(-1, -1, 3)
                _away(f'{case}: infill residual', (of.body_markers_rec - markers[0:T])[occluded].abs(),
                      m_pos[0:T, None, None].expand_as(occluded)[occluded])
            if w['motion_infill_contact_weight'] > 0:
                vel30 = (vw[1:] - vw[:-1]) * 30
                for k, name in enumerate(('left_heel', 'right_heel', 'left_toe', 'right_toe')):
                    lab = of.contact_lbl_rec[:, k] == 1
                    s = torch.norm(vel30[:, of.ids[name], :][lab], dim=-1)
                    _away(f'{case}: contact speed of {name} > {thr["contact"]}', (s - thr['contact']).abs(),
                          (30 * math.sqrt(3) * m_pair[lab])[:, None].expand_as(s))


def amass_margins(case, of, verts, m_pos):
    """`of`: the float64 AmassFitOracle, `verts` its vertices, `m_pos` [B] the position margins of the case"""
    w = of.w
    with default_f64(), torch.no_grad():
        v = verts.detach()
        P = float(v.abs().max())
        assert P < P_MAX, (case, P)
        if w['rec_markers'] > 0:
            r = (v[:, of.ids['markers67'], :] - of.markers_rec).abs()
            _away(f'{case}: marker residual', r, m_pos[:, None, None].expand_as(r))
        if w['contact_vel'] > 0:
            vel = (v[1:] - v[:-1]) * 30
            m_pair = m_pos[:-1] + m_pos[1:]
            for k, name in enumerate(('left_heel', 'right_heel', 'left_toe', 'right_toe')):
                lab = of.contact[0:-1, k] == 1
                s = torch.norm(vel[:, of.ids[name], :][lab], dim=-1)
                _away(f'{case}: contact speed of {name} > 0.1', (s - 0.1).abs(), (30 * math.sqrt(3) * m_pair[lab])[:, None].expand_as(s))


# ---------------------------------------------------------------------------------------------------------------------------
# PROX

def one_term_weights(on, base=S3_WEIGHTS):
    w = {k: 0.0 for k in WEIGHT_ORDER if k != 'bending_prior_weight'}            # bending follows body_pose inside both engines
    w.update(hand_weight=base['hand_weight'], face_weight=base['face_weight'])  # the joint weights are no loss weights: kept
    for k in on:
        w[k] = SHAPE_WEIGHT if k == 'shape_weight' else base[k]
    return w


def _prox_problem(case, B=14):
    mv = CASE_MOVES.get(case, {})
    prob = ge.prox_small_problem(B=B, stage='S3', seed=mv.get('seed', 5))
    if 'seq' in mv:               # another synthetic sequence, placed like prox_small_problem places its own (sequence 4)
        from lemo_amd import synthetic
        seq = synthetic.make_synthetic_sequence(mv['seq'], B=B)['init_params']
        prob['params'].update(betas=np.repeat(seq[:1, 6:16], B, 0), global_orient=seq[:, 3:6].copy(),
                              transl=seq[:, 0:3] + np.array([0, 0, 2.5], np.float32), left_hand_pose=seq[:, 48:60].copy(),
                              right_hand_pose=seq[:, 60:72].copy(), pose_embedding=seq[:, 16:48].copy())
    return prob


STATIC_THRESHOLDS = dict(fric_vn=-1e-9)
"""the static window's oracles test ``v_z < -1e-9`` in place of ``v_z < 0``: their batched products leave +-2e-16 (float64) / +-1e-7 (float32) where the
engine, which runs the same code on every frame, has exactly 0; read as downward motion that noise would put arbitrary vertices into the mean"""


def _prox_refs(case, prob, first, thresholds=None):
    """float32 and float64 oracle closures + the margin check -> (losses64, grads32, grads64)"""
    def grads(o):
        out = {}
        for n in PROX_GROUPS:
            p = o.pose_embedding if n == 'pose_embedding' else o.p[n]
            out[n] = (torch.zeros_like(p) if p.grad is None else p.grad).detach().double()
        return out
    o32s = [ge.prox_oracle_for(prob if k == 0 else dict(prob, vposer_w=permuted_decoder(prob['vposer_w'], k)), first_batch_flag=first)
            for k in range(N_ORDERS + 1)]
    o64 = prox_fit_oracle_f64(prob, first_batch_flag=first)
    if thresholds:
        from oracle.prox_oracle import THRESHOLDS
        for o in o32s + [o64]:
            o.thresholds = dict(THRESHOLDS, **thresholds)
    for o in o32s:
        o.closure()
    with default_f64():
        ld64 = {k: _f(v) for k, v in o64.closure().items()}
        with torch.no_grad():
            v64 = o64._body(True)[0]
    with torch.no_grad():
        more = [ge.prox_oracle_for(dict(prob, vposer_w=permuted_decoder(prob['vposer_w'], k)), first_batch_flag=first)
                for k in range(N_ORDERS + 1, N_POS_ORDERS + 1)]
        m_pos = position_margins(case, [o._body(True)[0] for o in o32s + more], v64)
    prox_margins(case, o64, m_pos, prob)
    g32, g64 = grads(o32s[0]), grads(o64)
    yardstick_is_no_luck(case, largest_err(g32, g64), [largest_err(grads(o), g64) for o in o32s[1:]])
    return ld64, g32, g64


def _prox_engine(lib, dev, prob, first):
    eng, _ = ge.prox_engine_for(prob, dev, first_batch_flag=first, lib=_lib_arg(lib))
    return eng


def check_prox_term(lib, dev, case):
    on, entry = PROX_TERMS[case]
    prob = _prox_problem(case)
    prob['weights'] = one_term_weights(on)
    ld64, g32, g64 = _prox_refs(case, prob, True)
    assert ld64['total_loss'] > 0 and (entry is None or ld64[entry] > 0), (case, ld64)      # the term is live in this problem
    eng = _prox_engine(lib, dev, prob, True)
    ld = eng.closure()
    for k in LOSS_KEYS:
        if k == 'total_loss' or k == entry:
            _rel_close(ld[k], ld64[k], f'{case} {k}')
        else:
            assert ld[k] == 0.0 and ld64[k] == 0.0, (case, k, ld[k], ld64[k])
    gate_groups('prox ' + case, eng.grads(), g32, g64)
    if case == 'shape':
        assert all(float(v.abs().max()) == 0.0 for v in g64.values())


def _check_all_terms(lib, dev, case, prob, first, zero_entries=(), thresholds=None):
    ld64, g32, g64 = _prox_refs(case, prob, first, thresholds)
    eng = _prox_engine(lib, dev, prob, first)
    ld = eng.closure()
    for k in LOSS_KEYS:
        if k in zero_entries:
            assert ld[k] == 0.0 and ld64[k] == 0.0, (case, k, ld[k], ld64[k])
        else:
            _rel_close(ld[k], ld64[k], f'{case} {k}')               # (an entry that is 0.0 in float64 must be 0.0: the bound is relative)
    g = eng.grads()
    gate_groups('prox ' + case, g, g32, g64)
    return eng, g, g64


def check_prox_window(lib, dev, B):
    """a later window of B frames: the first int(0.15 B) frames are frozen"""
    case = f'B{B}'
    prob = _prox_problem(case, B=B)
    # copies: on the CPU the engine steps the very arrays it is given
    start = {n: torch.from_numpy(np.array(prob['params'][n], np.float32).reshape(B, d)) for n, d in ENGINE_PARAMS}
    eng, g, g64 = _check_all_terms(lib, dev, case, prob, False)
    erase_n = int(B * 0.15)
    assert erase_n >= 1
    for n in PROX_GROUPS:
        assert float(g[n][:erase_n].abs().max()) == 0.0 and float(g64[n][:erase_n].abs().max()) == 0.0, (case, n)
    eng.step(1, use_graph=False)
    moved = 0
    for n, d in ENGINE_PARAMS:
        p0, p1 = start[n], eng.P[n].detach().cpu()
        assert torch.equal(p1[:erase_n].view(torch.int32), p0[:erase_n].view(torch.int32)), f'{case} {n}: a frozen frame moved'
        # Adam's first step from zero state moves every entry with a non-zero gradient by lr: the first free frame must have left
        free = g64[n][erase_n] != 0
        assert not bool((p1[erase_n] == p0[erase_n])[free].any()), f'{case} {n}: frame {erase_n} is free and did not move'
        moved += int(free.sum())
    assert moved > 0 and int(eng.step_ctr.item()) == 1 and eng.nonfinite_step() == 0


def check_prox_empty(lib, dev, case):
    prob = _prox_problem(case)
    zero = ()
    if case == 'sdf_plus_10':                     # no penetration and no friction contact
        prob['sdf'] = (prob['sdf'] + np.float32(10.0)).astype(np.float32)
        zero = ('sdf_penetration_loss', 'loss_fric_tangent', 'loss_fric_normal')
    elif case == 'no_contact_label':
        prob['infill'] = dict(prob['infill'], contact_lbl_rec=np.zeros_like(prob['infill']['contact_lbl_rec']))
        zero = ('motion_infill_contact_loss',)
    elif case == 'static_window':                 # every frame carries frame 0's parameters: all velocities are exactly 0
        prob['params'] = {k: np.repeat(np.asarray(v)[:1], prob['B'], 0).copy() for k, v in prob['params'].items()}
        zero = ('loss_fric_tangent', 'loss_fric_normal', 'motion_infill_contact_loss')
    elif case == 'sdf_weight_0':
        prob['weights'] = dict(prob['weights'], sdf_penetration_weight=0.0)
        zero = ('sdf_penetration_loss',)
    elif case == 'mask_all_ones':                 # rec given, nothing occluded: the host turns use_infill off (the oracle's :176 branch)
        prob['infill'] = dict(prob['infill'], marker_mask=np.ones_like(prob['infill']['marker_mask']))
        zero = ('motion_infill_loss', 'motion_infill_contact_loss')
    else:
        raise KeyError(case)
    eng, g, _ = _check_all_terms(lib, dev, case, prob, False, zero_entries=zero, thresholds=STATIC_THRESHOLDS if case == 'static_window' else None)
    if case == 'mask_all_ones':
        assert not eng.use_infill
    for n in PROX_GROUPS:
        assert torch.isfinite(g[n]).all(), (case, n)


def check_prox_many_friction_vertices(lib, dev):
    """300 friction vertices: the special set S exceeds 256 and prox_sparse_kernel runs a second blockIdx.y"""
    case = 'fric300'
    prob = _prox_problem(case)
    perm = np.random.default_rng(1).permutation(prob['V'])         # prox_small_problem's own permutation: its fric_ids are perm[40:70]
    assert np.array_equal(perm[40:70], prob['fric_ids'])
    prob['fric_ids'] = perm[40:340]
    eng, _, _ = _check_all_terms(lib, dev, case, prob, False)
    assert int(eng._t['s_vid'].numel()) > 256


def check_prox_refusals(lib, dev):
    """lemo_prox_create: B < 10, and use_infill with T > B - 1"""
    with pytest.raises(_hip.LemoHipError):
        _prox_engine(lib, dev, _prox_problem('refusal', B=9), True)
    prob = _prox_problem('refusal')
    eng = _prox_engine(lib, dev, prob, True)
    assert eng.use_infill and eng.desc.T == prob['B'] - 1
    d = _hip.ProxDesc()
    C.memmove(C.byref(d), C.byref(eng.desc), C.sizeof(d))
    h = lib.prox_create(C.byref(d))                                  # the copy itself is accepted ...
    assert h
    lib.prox_destroy(h)
    d.T = prob['B']                                                  # ... and one infill frame too many is not
    h = lib.prox_create(C.byref(d))
    if h:
        lib.prox_destroy(h)
    assert not h, 'lemo_prox_create accepted use_infill with T > B - 1'


# ---------------------------------------------------------------------------------------------------------------------------
# AMASS

def _amass_problem(case, **kw):
    mv = CASE_MOVES.get(case, {})
    prob = ge.small_problem(seed=mv.get('seed', 5), **kw)
    if 'seq' in mv:               # another synthetic sequence in place of small_problem's own (sequence 3)
        from lemo_amd import synthetic
        prob['seq'] = synthetic.make_synthetic_sequence(mv['seq'], B=prob['B'])
    return prob


def _amass_refs(case, prob, w):
    gr = lambda o: {n: (torch.zeros_like(getattr(o, n)) if getattr(o, n).grad is None else getattr(o, n).grad).detach().double() for n in AMASS_GROUPS}
    o32s, v32s = [], []
    for k in range(N_ORDERS + 1):
        o, mk = ge.oracle_for(prob if k == 0 else dict(prob, vposer_w=permuted_decoder(prob['vposer_w'], k)), weights=w)
        if k == 0:
            markers = mk
        else:
            o.markers_rec = o32s[0].markers_rec           # one target for every order (oracle_for decodes it with the weights it is given)
        tot, _, _, v = o.losses()
        tot.backward()
        o32s.append(o)
        v32s.append(v)
    o64 = amass_fit_oracle_f64(prob['model'], prob['vposer_w'], prob['enc_w'], prob['ids'], prob['Xmean'], prob['Xstd'],
                               prob['seq']['init_params'], markers, prob['seq']['contact_lbl'], weights=w,
                               extra_joint_ids=list(range(21)) if prob['V'] < 9930 else None)
    with default_f64():
        tot64, parts64, _, verts64 = o64.losses()
        tot64.backward()
    with torch.no_grad():
        for k in range(N_ORDERS + 1, N_POS_ORDERS + 1):
            o, _ = ge.oracle_for(dict(prob, vposer_w=permuted_decoder(prob['vposer_w'], k)), weights=w)
            v32s.append(o.losses()[3])
    amass_margins(case, o64, verts64, position_margins(case, v32s, verts64))
    g32, g64 = gr(o32s[0]), gr(o64)
    yardstick_is_no_luck(case, largest_err(g32, g64), [largest_err(gr(o), g64) for o in o32s[1:]])
    return markers, _f(tot64), {k: _f(v) for k, v in parts64.items()}, g32, g64


def _amass_fitter(lib, dev, prob, w, markers, **kw):
    fit = AmassTemporalFitter(prob['model'], prob['vposer_w'], prob['enc_w'], prob['ids'], prob['Xmean'], prob['Xstd'], prob['B'], dev,
                              weights=w, lib=lib, **kw)
    fit.load_sequence(prob['seq']['init_params'], markers, prob['seq']['contact_lbl'])
    return fit


PART_OF = dict(rec_markers='marker', contact_vel='contact', smooth='smooth', vposer='vposer', shape='shape', hand='hand')


def check_amass_term(lib, dev, term, full, large=False):
    """one of the three vertex terms alone (or, `large`, the three together on the problem whose loss-carrying set exceeds 1024 vertices:
    dverts_assemble + the dense LBS backward) through forward / backward / grads()"""
    case = ('large ' if large else '') + f'{term} full={int(full)}'
    prob = _amass_problem(case, **(dict(B=12, V=1300, foot=262) if large else {}))
    w = {k: 0.0 for k in LOSS_WEIGHTS}
    for k in (AMASS_TERMS if large else (term,)):
        w[k] = LOSS_WEIGHTS[k]
    markers, tot64, parts64, g32, g64 = _amass_refs(case, prob, w)
    fit = _amass_fitter(lib, dev, prob, w, markers, full_vertices=full)
    assert not large or fit.n > 1024
    fit.forward()
    fit.backward()
    L = fit.losses()
    for k in (AMASS_TERMS if large else (term,)):
        assert parts64[PART_OF[k]] > 0
        _rel_close(L[PART_OF[k]], parts64[PART_OF[k]], f'{case} {PART_OF[k]}')
    _rel_close(L['total'], tot64, f'{case} total')
    gate_groups('amass ' + case, fit.grads(), g32, g64)


def check_amass_prior(lib, dev, prior):
    """one L2 prior alone: the gradient fit_tail_kernel adds, read from exp_avg after one step from zero state"""
    case = f'prior {prior}'
    prob = _amass_problem(case)
    w = {k: 0.0 for k in LOSS_WEIGHTS}
    w[prior] = LOSS_WEIGHTS[prior]
    markers, tot64, parts64, g32, g64 = _amass_refs(case, prob, w)
    fit = _amass_fitter(lib, dev, prob, w, markers, full_vertices=False)
    fit.step(1, use_graph=False)
    st = fit.save_state()
    assert int(st['step'].item()) == 1
    got = {n: st['m_' + n].detach().cpu().double() / float(np.float32(0.1)) for n in AMASS_GROUPS}
    L = fit.losses()
    _rel_close(L[PART_OF[prior]], parts64[PART_OF[prior]], f'{case} {PART_OF[prior]}')
    _rel_close(L['total'], tot64, f'{case} total')
    if prior == 'shape':
        assert all(float(v.abs().max()) == 0.0 for v in g64.values())
    gate_groups('amass ' + case, got, g32, g64, extra=FLOOR)


def check_amass_prior_per_frame(lib, dev):
    """per_frame=True, B = 3: every row is a fit of its own and the priors' means run over one row (Bn = 1)"""
    from oracle import lemo_oracle as O
    case = 'prior per_frame'
    B = 3
    prob = _amass_problem(case, B=B)
    w = dict({k: 0.0 for k in LOSS_WEIGHTS}, vposer=LOSS_WEIGHTS['vposer'], hand=LOSS_WEIGHTS['hand'])
    _, markers = ge.oracle_for(prob, weights=w)
    extra = list(range(21)) if prob['V'] < 9930 else None
    so = O.SmplxOracle(prob['model'], extra_joint_ids=extra)
    vwt = {k: torch.from_numpy(v) for k, v in prob['vposer_w'].items()}
    ids = np.asarray(prob['ids']['markers67'])
    init = prob['seq']['init_params']
    r32 = [PLO.perframe_iteration(so, vwt, ids, init[t], markers[t], weights=w) for t in range(B)]
    r64 = [perframe_iteration_f64(prob['model'], prob['vposer_w'], ids, init[t], markers[t], weights=w, extra_joint_ids=extra) for t in range(B)]
    stack = lambda rs, k: torch.from_numpy(np.concatenate([np.asarray(r[k]).reshape(1, -1) for r in rs])).double()
    g32 = {n: stack(r32, 'g_' + n) for n in AMASS_GROUPS}
    g64 = {n: stack(r64, 'g_' + n) for n in AMASS_GROUPS}
    fit = _amass_fitter(lib, dev, prob, w, markers, full_vertices=False, per_frame=True)
    fit.step(1, use_graph=False)
    st = fit.save_state()
    got = {n: st['m_' + n].detach().cpu().double() / float(np.float32(0.1)) for n in AMASS_GROUPS}
    gate_groups('amass ' + case, got, g32, g64, extra=FLOOR)
