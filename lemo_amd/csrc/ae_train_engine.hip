// Native training step of the motion-infilling autoencoder as train_infill_prior.py:185-203 trains it: ONE parameter set over a
// batch of bs images (models/AE.py, AE(downsample=True, in_channel=4, kernel=3), body_mode 'local_markers_4chan'):
//   rec = AE(x)                                   x [bs][4][H][W]: the masked, reflect-padded clip image; y [bs][H][W]: the target
//   loss = w_body mean|y - rec| (rows < H - 5) + w_v mean|dy - drec| (same rows, column differences)
//        + w_c BCEWithLogits(rec, y) (the 5 bottom rows)
//   torch.optim.Adam(lr) with default betas / eps over all 40 tensors.
// The finetune engine (ae_engine.hip) runs K clips side by side with K parameter sets; here the batch images ride along the same
// launches' clip dimension with the parameters shared (weight stride 0, ae_conv's wcs):
//   * forward and backward-data: ae_conv, maxpool3s2_*, stuff2_fwd with nclip = bs (ae_conv_shape picks shapes for the bs images in flight);
//   * loss and adjoint: one launch writes d(rec) into channel 0 of the last layer's d(pre-activation), per-block loss partials and
//     Adam's device-side step counter; a one-block launch sums the partials in a fixed order;
//   * weight and bias gradients: ONE launch over all 20 layers (aet_wgrad_kernel: ae_wgrad_multi_kernel's wave tile with a loop over
//     the images of an image group).  K = bs x pixels is cut into AET_GROUPS image groups x the layer's pixel slabs; every (group,
//     slab) writes one partial tile, so the partial storage is AET_GROUPS x the finetune engine's per clip, whatever bs is;
//   * Adam + backward-pack rebuild: ae_adam_kernel, which sums those partials in (group, slab) order.
// No float atomics: every sum has a fixed order, so a graph replay, an eager run and a second engine give identical bits.
#include "ae_engine.hpp"
#include "train_epoch.hpp"

#include <cstring>
#include <new>

#define AET_GROUPS 8              // image groups of the weight-gradient reduction (at most; fewer when bs < 8)
#define AET_MAX_BS 128
#define AET_LOSS_BLOCK 256

namespace lemo {

// jobs: image 0's operands; partial [group][slab][9 cin cout], dbp [group][slab][2][cout]
struct AetWgradJobs { AeWgradJob j[AE_NLAYER]; int first[AE_NLAYER + 1]; int n; int bs, groups; size_t cs; };

// One wave = one 32 (ci) x 32 (co) tile, one kernel row, one pixel slab, one image group (blockIdx.y): the images of the group one
// after the other into the same accumulators (image order, then pixel order: deterministic).  Per image the loop is
// ae_wgrad_multi_kernel's (mode 0): three accumulators (dx = -1, 0, +1), one dY operand times three X operands out of a sliding
// 17-pixel window, the next 16 pixels' operands requested before the current ones' MFMAs.
__global__ void __launch_bounds__(64)
aet_wgrad_kernel(AetWgradJobs J) {
  int k = 0;
  while (k + 1 < J.n && (int)blockIdx.x >= J.first[k + 1]) ++k;               // block -> layer (uniform)
  const AeWgradJob& q = J.j[k];
  int tile = (int)blockIdx.x - J.first[k];                         // (slab, co tile, ci tile, kernel row)
  const int lane = threadIdx.x;
  const int Wp = q.W + 2, HWp = (q.H + 2) * Wp;
  const int i = lane & 31, kk = lane >> 5;
  const int cin = q.cin, cout = q.cout;
  const int cot = cout >> 5, cit = (cin + 31) >> 5;
  const int r = tile % 3; tile /= 3;                               // kernel row dy = r - 1
  const int ct = tile % cit; tile /= cit;
  const int mt = tile % cot;
  const int slab = tile / cot;
  const int co = mt * 32 + i;
  int ci = ct * 32 + i;
  if (ci >= cin) ci = cin - 1;                                     // rows past cin are computed and never stored
  const int grp = blockIdx.y;
  const int c0 = grp * J.bs / J.groups, c1 = (grp + 1) * J.bs / J.groups;
  const int Q1 = (q.H + 1) * Wp;                                   // interior rows: padded pixels [Wp, (H + 1) Wp)
  const int qs = Wp + slab * q.slab_len;
  const int qe = qs + q.slab_len < Q1 ? qs + q.slab_len : Q1;      // (host: qs < Q1)
  const int off = (r - 1) * Wp + kk - 1;
  f32x16 acc0, acc1, acc2;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; acc2[e] = 0.f; }
  float bsum = 0.f;
  float b[2][8], xw[2][17];
  for (int c = c0; c < c1; ++c) {
    const size_t img = (size_t)c * J.cs;
    const float* bp = q.dy + img + ((size_t)(co >> 3) * HWp) * 8 + (co & 7);
    const float* ap = q.x + img + ((size_t)(ci >> 3) * HWp) * 8 + (ci & 7);
#define WG_LOAD(SET, QB)                                                                           \
  {                                                                                                \
    const float* bq = bp + (std::ptrdiff_t)((QB) + kk) * 8;                                        \
    const float* aq = ap + (std::ptrdiff_t)((QB) + off) * 8;                                       \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) b[SET][u] = bq[16 * u];                          \
    _Pragma("unroll") for (int t = 0; t < 17; ++t) xw[SET][t] = aq[8 * t];                         \
    if ((QB) + 16 > qe) {                      /* last group of the slab: pixels past its end */    \
      _Pragma("unroll") for (int u = 0; u < 8; ++u) if ((QB) + 2 * u + kk >= qe) b[SET][u] = 0.f;  \
    }                                                                                              \
  }
#define WG_MFMA(SET)                                                                               \
  _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                  \
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xw[SET][2 * u], b[SET][u], acc0, 0, 0, 0);         \
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xw[SET][2 * u + 1], b[SET][u], acc1, 0, 0, 0);     \
    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(xw[SET][2 * u + 2], b[SET][u], acc2, 0, 0, 0);     \
    bsum += b[SET][u];                                                                             \
  }
    WG_LOAD(0, qs)
    for (int qb = qs; qb < qe; qb += 32) {
      if (qb + 16 < qe) { WG_LOAD(1, qb + 16) }
      __builtin_amdgcn_sched_barrier(0);
      WG_MFMA(0)
      __builtin_amdgcn_sched_barrier(0);
      if (qb + 16 < qe) {
        if (qb + 32 < qe) { WG_LOAD(0, qb + 32) }
        __builtin_amdgcn_sched_barrier(0);
        WG_MFMA(1)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#undef WG_LOAD
#undef WG_MFMA
  }
  // D: col = lane & 31 -> co, rows (e & 3) + 8 (e >> 2) + 4 kk -> ci, stored in the forward pack wt[tap][ci/8][co][8]
  const size_t part = (size_t)grp * q.nslab + slab;
  float* outp = q.partial + part * (9 * (size_t)cin * cout);
  const int CG = cin >> 3;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int cg = ct * 4 + qd;
    if (cg < CG) {
      float* o = outp + (((size_t)(3 * r) * CG + cg) * cout + co) * 8 + 4 * kk;
      const size_t tap_stride = (size_t)CG * cout * 8;
      st4(o, make_float4(acc0[4 * qd], acc0[4 * qd + 1], acc0[4 * qd + 2], acc0[4 * qd + 3]));
      st4(o + tap_stride, make_float4(acc1[4 * qd], acc1[4 * qd + 1], acc1[4 * qd + 2], acc1[4 * qd + 3]));
      st4(o + 2 * tap_stride, make_float4(acc2[4 * qd], acc2[4 * qd + 1], acc2[4 * qd + 2], acc2[4 * qd + 3]));
    }
  }
  if (r == 1 && ct == 0) q.dbp[(part * 2 + kk) * cout + co] = bsum;
}

// d(loss)/d(rec) and the loss partials of one block of pixels of one image (blockIdx.y).  rec: channel 0 of the last layer's output
// (CG8P), y: [bs][H][W].  Body rows r < H - 5: L1 and the velocity L1 over column differences; the 5 bottom rows: BCE with logits,
// evaluated as torch does.  step: thread 0 of the launch advances Adam's step counter and bias corrections (graph replay).
struct AetLossArgs {
  const float* rec; const float* y; float* dpre; float* part; float* ctr;
  int H, W; size_t cs; double lr; int step;
  float cb, cv, cc;                 // w_body / N1, w_v / N2, w_c / N3 (the adjoint's coefficients)
};
__device__ __forceinline__ float aet_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ void __launch_bounds__(AET_LOSS_BLOCK)
aet_loss_kernel(AetLossArgs A) {
  __shared__ float red[AET_LOSS_BLOCK / 64];
  const int c = blockIdx.y, H = A.H, W = A.W, Wp = W + 2;
  const float* rec = A.rec + (size_t)c * A.cs;
  float* dpre = A.dpre + (size_t)c * A.cs;
  const float* y = A.y + (size_t)c * H * W;
  if (A.step && c == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    int* ci = reinterpret_cast<int*>(A.ctr);
    const int step = ci[0] + 1;
    ci[0] = step;
    const AdamCoef ac = adam_coef_t(step, A.lr);
    A.ctr[1] = ac.neg_step;
    A.ctr[2] = ac.bc2s;
  }
  const int p = blockIdx.x * AET_LOSS_BLOCK + threadIdx.x;
  float lb = 0.f, lv = 0.f, lc = 0.f;
  if (p < H * W) {
    const int row = p / W, t = p - row * W;
    const size_t o = (size_t)((row + 1) * Wp + t + 1) * 8;
    const float l = rec[o], yy = y[p];
    float g;
    if (row < H - 5) {
      const float d = l - yy;
      lb = fabsf(d);
      g = A.cb * aet_sign(d);
      float s_prev = 0.f, s_cur = 0.f;                             // s_t = sign(drec_t - dy_t), 0 outside 0 .. W - 2
      if (t + 1 < W) {
        const float dv = (rec[o + 8] - l) - (y[p + 1] - yy);
        lv = fabsf(dv);
        s_cur = aet_sign(dv);
      }
      if (t > 0) s_prev = aet_sign((l - rec[o - 8]) - (yy - y[p - 1]));
      g += A.cv * (s_prev - s_cur);
    } else {
      const float m = fmaxf(-l, 0.f);
      lc = (1.f - yy) * l + m + logf(expf(-m) + expf(-l - m));
      g = A.cc * (1.f / (1.f + expf(-l)) - yy);
    }
    dpre[o] = g;
  }
  lb = block_sum(lb, red);
  lv = block_sum(lv, red);
  lc = block_sum(lc, red);
  if (threadIdx.x == 0) {
    float* q = A.part + ((size_t)c * gridDim.x + blockIdx.x) * 3;
    q[0] = lb; q[1] = lv; q[2] = lc;
  }
}

// the partials in block order -> losses {L_body, L_v, L_c, total}
__global__ void __launch_bounds__(256)
aet_loss_reduce_kernel(const float* __restrict__ part, int nblk, float inv1, float inv2, float inv3, float wb, float wv, float wc,
                       float* __restrict__ losses) {
  __shared__ float red[4];
  float s[3] = {0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < nblk; b += 256)
    for (int k = 0; k < 3; ++k) s[k] += part[(size_t)b * 3 + k];
  for (int k = 0; k < 3; ++k) s[k] = block_sum(s[k], red);
  if (threadIdx.x == 0) {
    const float l0 = s[0] * inv1, l1 = s[1] * inv2, l2 = s[2] * inv3;
    losses[0] = l0; losses[1] = l1; losses[2] = l2;
    losses[3] = wb * l0 + wv * l1 + wc * l2;
  }
}

// x [bs][4][H][W] -> CG8P channels 0..3 of each image's x8; y [bs][H][W] -> the engine's copy
__global__ void __launch_bounds__(256)
aet_stage_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ x8, float* __restrict__ ybuf, int H, int W, size_t cs) {
  const int c = blockIdx.y, HW = H * W;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 5 * HW) return;
  if (t < 4 * HW) {
    const int ch = t / HW, p = t - ch * HW, row = p / W, col = p - row * W;
    x8[(size_t)c * cs + (size_t)((row + 1) * (W + 2) + col + 1) * 8 + ch] = x[(size_t)c * 4 * HW + t];
  } else {
    ybuf[(size_t)c * HW + t - 4 * HW] = y[(size_t)c * HW + t - 4 * HW];
  }
}

// channel 0 of each image's reconstruction -> rec [bs][H][W]
__global__ void __launch_bounds__(256)
aet_rec_kernel(const float* __restrict__ act, float* __restrict__ rec, int H, int W, size_t cs) {
  const int c = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int row = p / W, col = p - row * W;
  rec[(size_t)c * H * W + p] = act[(size_t)c * cs + (size_t)((row + 1) * (W + 2) + col + 1) * 8];
}

// the step's summed gradient in the packed parameter layout: ae_adam_kernel's reduction (same order, same bits), no update
__global__ void __launch_bounds__(256)
aet_grad_kernel(AeAdamArgs A, float* __restrict__ gpk) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.n_all) return;
  float g = 0.f;
  if (idx < A.n_w) {
    int k = 0;
    while (k + 1 < AE_NLAYER && idx >= A.L[k + 1].w_off) ++k;
    const AeAdamLayer& q = A.L[k];
    const int i = idx - q.w_off;
    const int c8 = i & 7, co = (i >> 3) & ((1 << q.cout_lg) - 1);
    const int cg = (i >> (3 + q.cout_lg)) & ((1 << q.cin_lg) - 1);
    const int n_w = 9 << (q.cin_lg + 3 + q.cout_lg);
    if (cg * 8 + c8 < q.cin && co < q.cout)
      for (int s = 0; s < q.nslab; ++s) g += q.partial[(size_t)s * n_w + i];
  } else {
    const int bi = idx - A.n_w;
    int k = 0;
    while (k + 1 < AE_NLAYER && bi >= A.L[k + 1].b_off) ++k;
    const AeAdamLayer& q = A.L[k];
    const int co = bi - q.b_off, cop = 1 << q.cout_lg;
    if (co < q.cout)
      for (int s = 0; s < 2 * q.nslab; ++s) g += q.dbp[(size_t)s * cop + co];
  }
  gpk[idx] = g;
}

// ---------------------------------------------------------------------------------------------------------------------
// the engine
// ---------------------------------------------------------------------------------------------------------------------
struct AetEngine : AeNet, TrainReplay {       // (the network's buffers are image 0's; image c's are `c * cs` floats further)
  int bs = 1, groups = 1;
  double lr = 0.0; float lr_f = 0.f, w_body = 10.f, w_v = 10.f, w_c = 1.f;
  int nblk = 0;
  // shared by the batch
  float *theta = nullptr, *m = nullptr, *v = nullptr, *wb = nullptr, *dbp = nullptr, *part = nullptr, *zero_bias = nullptr,
        *amax = nullptr, *gpk = nullptr, *lpart = nullptr, *ybuf = nullptr;
  size_t cs = 0;
};

static bool aet_shape_ok(int H, int W, int bs) {
  return H >= 6 && W >= 2 && (long)H * W <= (1l << 22) && bs >= 1 && bs <= AET_MAX_BS;
}

// the same routine sizes the workspace (base == nullptr) and carves it: the shared region, then bs per-image regions
static void aet_layout(AetEngine* e, int H0, int W0, int bs, float* base, size_t* total) {
  e->bs = bs;
  e->groups = bs < AET_GROUPS ? bs : AET_GROUPS;
  const AePartials np = ae_net_layers(*e, H0, W0, 1, e->groups);
  e->nblk = bs * ((H0 * W0 + AET_LOSS_BLOCK - 1) / AET_LOSS_BLOCK);
  Bump B{base};
  e->theta = B.take(e->n_w + e->n_b); e->m = B.take(e->n_w + e->n_b); e->v = B.take(e->n_w + e->n_b); e->gpk = B.take(e->n_w + e->n_b);
  e->wb = B.take(e->n_wb); e->dbp = B.take(np.dbp); e->part = B.take(np.part);
  e->zero_bias = B.take(256); e->ctr = B.take(64); e->amax = B.take(64); e->losses = B.take(64);
  e->lpart = B.take((size_t)e->nblk * 3); e->ybuf = B.take((size_t)bs * H0 * W0);
  const size_t shared = B.off;
  Bump I{base ? base + shared : nullptr};
  ae_net_carve_image(*e, I);
  e->cs = I.off;
  *total = shared + (size_t)bs * I.off;
}

// every launch carries the batch (clip dimension = image) with one parameter set (weight stride 0) and no split-f16 scale slots
static auto aet_conv_of(AetEngine* e, hipStream_t s) {
  return [e, s](const AeConvSite&, const float* in, const float* wt, const float* bias, const float* aux, float* out, const AeGeo& g,
                int cin, int cout, int epi) { return ae_conv(in, wt, bias, aux, out, g, cin, cout, epi, s, 0, 0, 0, e->bs, e->cs, nullptr, 0); };
}

static int aet_forward(AetEngine* e, hipStream_t s) { return ae_net_forward(*e, e->theta, AeBatch{e->bs, e->cs, s}, aet_conv_of(e, s)); }

static int aet_loss(AetEngine* e, bool step, hipStream_t s) {
  const int H = e->H[0], W = e->W[0];
  const double n1 = (double)e->bs * (H - 5) * W, n2 = (double)e->bs * (H - 5) * (W - 1), n3 = (double)e->bs * 5 * W;
  AetLossArgs A{e->act[19], e->ybuf, e->dp[19], e->lpart, e->ctr, H, W, e->cs, e->lr, step ? 1 : 0,
                (float)(e->w_body / n1), (float)(e->w_v / n2), (float)(e->w_c / n3)};
  hipLaunchKernelGGL(aet_loss_kernel, dim3(e->nblk / e->bs, e->bs), dim3(AET_LOSS_BLOCK), 0, s, A);
  CHK((int)hipGetLastError());
  hipLaunchKernelGGL(aet_loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)e->lpart, e->nblk, (float)(1.0 / n1), (float)(1.0 / n2),
                     (float)(1.0 / n3), e->w_body, e->w_v, e->w_c, e->losses);
  return (int)hipGetLastError();
}

// the optimiser sums a layer's partials over (group, slab); one parameter set: no clip stride
static AeAdamArgs aet_adam_args(const AetEngine* e) {
  return ae_adam_args(*e, e->part, e->dbp, e->groups, e->theta, e->m, e->v, e->wb, e->ctr, e->amax, e->lr_f, 0);
}

static int aet_wgrad(AetEngine* e, hipStream_t s) {
  AetWgradJobs J;
  const AeWgradCount c = ae_wgrad_jobs(*e, e->part, e->dbp, J.j, J.first);
  J.n = c.n; J.bs = e->bs; J.groups = e->groups; J.cs = e->cs;
  hipLaunchKernelGGL(aet_wgrad_kernel, dim3(c.nb, e->groups), dim3(64), 0, s, J);
  return (int)hipGetLastError();
}

static int aet_train_step(AetEngine* e, hipStream_t s) {
  CHK(aet_forward(e, s));
  CHK(aet_loss(e, true, s));
  CHK(ae_net_backward_data(*e, e->wb, e->zero_bias, AeBatch{e->bs, e->cs, s}, aet_conv_of(e, s)));
  CHK(aet_wgrad(e, s));
  return ae_adam_launch(aet_adam_args(e), 1, s);
}

static int aet_stage(AetEngine* e, const float* x, const float* y, hipStream_t s) {
  const int H = e->H[0], W = e->W[0];
  hipLaunchKernelGGL(aet_stage_kernel, dim3((5 * H * W + 255) / 256, e->bs), dim3(256), 0, s, x, y, e->x8, e->ybuf, H, W, e->cs);
  return (int)hipGetLastError();
}

// ---- the loop level: an epoch of different batches assembled on the device (train_epoch.hpp)
// the descriptor's shape rules (the index VALUES live on the device: the caller validates them, lemo_amd/infill_train.py does)
static int aet_epoch_block(const AetEngine* e, const lemo_aetrain_epoch_desc* d, EpochBlock* B) {
  if (!d || !d->data || !d->idx || d->n_clips < 1 || d->n_steps < 1) return LEMO_ERR_ARG;
  const int dd = e->H[0] - 2, T = e->W[0] - 16;
  if (T < 9) return LEMO_ERR_SHAPE;                                 // reflect padding by 8 needs more than 8 frames
  if (d->recipe != LEMO_MASK_NONE && d->recipe != LEMO_MASK_RANDOM && d->recipe != LEMO_MASK_PROX) return LEMO_ERR_ARG;
  if (d->recipe != LEMO_MASK_NONE && dd != 208) return LEMO_ERR_ARG;             // 3 pelvis + 3 x 67 marker + 4 contact rows
  if (d->recipe == LEMO_MASK_RANDOM && !d->marker_ids) return LEMO_ERR_ARG;
  if (d->recipe == LEMO_MASK_PROX && (!d->masks || !d->mask_idx || d->n_masks < 1 || d->mask_len < T)) return LEMO_ERR_ARG;
  *B = EpochBlock{d->data, d->idx, d->marker_ids, d->masks, d->mask_idx, d->log, d->n_clips, d->n_masks, d->mask_len, d->n_steps,
                  d->recipe, 0};
  return 0;
}

// one step of an epoch: every kernel reads the step from the device-side cursor
static int aet_epoch_step(AetEngine* e, bool train, hipStream_t s) {
  CHK(aet_assemble(EpochBlock{}, ep_block(e->ctr), 0, e->x8, e->cs, e->ybuf, e->bs, e->H[0], e->W[0], s));
  if (train) {
    CHK(aet_train_step(e, s));
  } else {
    CHK(aet_forward(e, s));
    CHK(aet_loss(e, false, s));
  }
  return ep_end(ep_block(e->ctr), e->losses, 4, s);
}

}  // namespace lemo

using namespace lemo;

extern "C" {

long long lemo_aetrain_ws_floats(int H, int W, int bs) {
  if (!aet_shape_ok(H, W, bs)) return 0;
  AetEngine e;
  size_t total = 0;
  aet_layout(&e, H, W, bs, nullptr, &total);
  return (long long)total;
}

void* lemo_aetrain_create(const lemo_aetrain_desc* d) {
  if (!d || !d->ws || !aet_shape_ok(d->H, d->W, d->bs) || !(d->lr > 0.f)) return nullptr;
  if (ae_conv_init()) return nullptr;                              // LDS opt-ins before any capture
  AetEngine* e = new (std::nothrow) AetEngine();
  if (!e) return nullptr;
  size_t total = 0;
  aet_layout(e, d->H, d->W, d->bs, d->ws, &total);
  if ((long long)total > d->ws_floats) { delete e; return nullptr; }
  e->lr_f = d->lr; e->lr = lr_decimal(d->lr);
  e->w_body = d->w_body; e->w_v = d->w_v; e->w_c = d->w_c;
  e->use_graph = d->use_graph;
  return e;
}

void lemo_aetrain_destroy(void* h) {
  AetEngine* e = (AetEngine*)h;
  if (!e) return;
  e->destroy_graphs();
  delete e;
}

int lemo_aetrain_load(void* h, const float* flat, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !flat) return LEMO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n_all = (size_t)e->n_w + e->n_b;
  CHK(ae_pack_launch(ae_pack_args(*e), false, flat, e->theta, e->wb, s));
  CHK((int)hipMemsetAsync(e->m, 0, sizeof(float) * n_all, s));          // a fresh optimizer
  CHK((int)hipMemsetAsync(e->v, 0, sizeof(float) * n_all, s));
  CHK((int)hipMemsetAsync(e->ctr, 0, sizeof(float) * 64, s));
  e->loaded = 1;
  return 0;
}

int lemo_aetrain_step(void* h, const float* x, const float* y, int n, float* losses, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !x || !y || n < 1) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  CHK(aet_stage(e, x, y, s));
  CHK(replay_or_run(&e->exec, e->use_graph, n, s, [&] { return aet_train_step(e, s); }));
  if (losses) CHK((int)hipMemcpyAsync(losses, e->losses, sizeof(float) * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

int lemo_aetrain_eval(void* h, const float* x, const float* y, float* losses, float* rec, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !x || !y || !losses) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  CHK(aet_stage(e, x, y, s));
  CHK(aet_forward(e, s));
  CHK(aet_loss(e, false, s));
  CHK((int)hipMemcpyAsync(losses, e->losses, sizeof(float) * 4, hipMemcpyDeviceToDevice, s));
  if (rec) {
    hipLaunchKernelGGL(aet_rec_kernel, dim3((e->H[0] * e->W[0] + 255) / 256, e->bs), dim3(256), 0, s, (const float*)e->act[19], rec,
                       e->H[0], e->W[0], e->cs);
    CHK((int)hipGetLastError());
  }
  return 0;
}

int lemo_aetrain_params(void* h, float* flat_out, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !flat_out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  return ae_pack_launch(ae_pack_args(*e), true, e->theta, flat_out, nullptr, (hipStream_t)stream);
}

int lemo_aetrain_grads(void* h, float* flat_out, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !flat_out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const AeAdamArgs A = aet_adam_args(e);
  hipLaunchKernelGGL(aet_grad_kernel, dim3((A.n_all + 255) / 256), dim3(256), 0, s, A, e->gpk);
  CHK((int)hipGetLastError());
  return ae_pack_launch(ae_pack_args(*e), true, e->gpk, flat_out, nullptr, s);
}

int lemo_aetrain_epoch(void* h, const lemo_aetrain_epoch_desc* d, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !d || !d->log) return LEMO_ERR_ARG;
  EpochBlock B;
  CHK(aet_epoch_block(e, d, &B));
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const bool train = d->train != 0;
  CHK(ep_begin(B, ep_block(e->ctr), s));
  return replay_or_run(&e->exec_ep[train], e->use_graph, d->n_steps, s, [&] { return aet_epoch_step(e, train, s); });
}

int lemo_aetrain_batch(void* h, const lemo_aetrain_epoch_desc* d, int step, float* x, float* y, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !x || !y) return LEMO_ERR_ARG;
  EpochBlock B;
  CHK(aet_epoch_block(e, d, &B));
  if (step < 0 || step >= d->n_steps) return LEMO_ERR_ARG;
  return aet_assemble_api(B, step, x, y, e->bs, e->H[0], e->W[0], (hipStream_t)stream);
}

long long lemo_aetrain_state_floats(void) {
  AeNet n;
  ae_net_layers(n, 8, 8, 1, 1);            // (the parameter count does not depend on the image size)
  return 3ll * n.n_flat + 2;
}

int lemo_aetrain_state_save(void* h, float* out, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const AePackArgs P = ae_pack_args(*e);
  CHK(ae_pack_launch(P, true, e->theta, out, nullptr, s));
  CHK(ae_pack_launch(P, true, e->m, out + e->n_flat, nullptr, s));
  CHK(ae_pack_launch(P, true, e->v, out + 2 * (size_t)e->n_flat, nullptr, s));
  return train_step_counter(e->ctr, out + 3 * (size_t)e->n_flat, true, s);
}

int lemo_aetrain_state_load(void* h, const float* in, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !in) return LEMO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const AePackArgs P = ae_pack_args(*e);
  // the moments take the parameters' packing; the backward pack it writes on the way goes to the gradient scratch (gpk holds
  // n_w + n_b >= n_wb floats and is rewritten by every lemo_aetrain_grads), then the parameters' own backward pack to wb
  CHK(ae_pack_launch(P, false, in + e->n_flat, e->m, e->gpk, s));
  CHK(ae_pack_launch(P, false, in + 2 * (size_t)e->n_flat, e->v, e->gpk, s));
  CHK(ae_pack_launch(P, false, in, e->theta, e->wb, s));
  CHK((int)hipMemsetAsync(e->ctr, 0, sizeof(float) * 64, s));
  CHK(train_step_counter(e->ctr, const_cast<float*>(in) + 3 * (size_t)e->n_flat, false, s));
  e->loaded = 1;
  return 0;
}

int lemo_aetrain_pool_winners(void* h, int block, unsigned char* out, void* stream) {
  AetEngine* e = (AetEngine*)h;
  if (!e || !out || block < 0 || block > 4) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  const size_t n = (size_t)e->L[2 * block + 1].cout_pad * e->H[block + 1] * e->W[block + 1];
  for (int c = 0; c < e->bs; ++c)                                  // (idx is carved in floats: image c's bytes are 4 c cs further)
    CHK((int)hipMemcpyAsync(out + c * n, e->idx[block] + 4 * (size_t)c * e->cs, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
