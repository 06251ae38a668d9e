// Training-step engine of the smoothness prior (models/AE_sep.py Enc + Dec with downsample=False, z_channel=64;
// train_smooth_prior.py:96-136): per step, for a batch of network inputs x [bs][H][W] (velocity image, reflect-padded),
//   z = Enc(x), rec = Dec(z), loss = w_rec mean|x - rec| + w_smooth mean((z[..., 1:] - z[..., :-1])^2), Adam over all 40 tensors.
//
// Launches of one step (bs images):
//   forward   1 pad + bs x (1 conv3x3_c1 + 9 conv3x3_mfma_lds) [Enc] + bs x 8 conv3x3_mfma_lds [Dec deconvs as convs with the
//             flipped / transposed pack] + 2 (decoder end: 32 -> 1 + lrelu; 1 -> 1 + L1 partials + d rec) + bs smooth_loss + 1 losses
//   backward  2 (decoder end adjoints) + 2 x 2 (1-channel weight gradients) + bs x 8 backward-data + 8 x 2 weight gradients [Dec]
//             + 1 add (d z from Dec + smoothness term) + bs x 9 backward-data + 9 x 2 + 2 weight gradients [Enc]
//   update    1 Adam (flat vector) + 1 repack (every conv pack from the updated fp32 weights)
// i.e. 36 bs + 48 launches, captured once as a graph when use_graph is set.  The fp32 parameters, Adam moments and gradients
// are one flat vector in the reference's state_dict order (Enc then Dec); layers 0 of Enc and 8, 9 of Dec read it directly.
#include "kernels.hpp"
#include "train_epoch.hpp"

#include <cstring>
#include <new>

namespace lemo {

static const int SP_ENC_CH[11] = {1, 32, 32, 64, 64, 64, 64, 64, 64, 64, 64};
static const int SP_DEC_IN[10] = {64, 64, 64, 64, 64, 64, 64, 32, 32, 1};
static const int SP_DEC_OUT[10] = {64, 64, 64, 64, 64, 64, 32, 32, 1, 1};

// conv view of a layer: forward maps cin -> cout channels (Dec: cin = nin, cout = nout); fwt / bwt: tap-major and channel-group-major
// packs of its forward and backward-data convolutions (null for the 1-channel layers, which read the flat weights)
struct SpLayer { int cin, cout, w_off, b_off; float *fwt, *fwt2, *bwt, *bwt2; };

struct SpEngine : TrainReplay {
  int H = 0, W = 0, bs = 0, n_param = 0;
  double lr = 0.0;
  float w_rec = 0.f, w_smooth = 0.f;
  size_t is = 0, i1 = 0;                // floats per image: CG8P buffer of 64 channels (all CG8P buffers use it) / plain padded image
  SpLayer enc[10] = {}, dec[10] = {};
  float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *lpart = nullptr, *spart = nullptr, *wsg = nullptr;
  float *xin = nullptr, *x0 = nullptr, *r1 = nullptr, *rec = nullptr, *drec = nullptr, *dpre8 = nullptr;
  float *act[11] = {}, *dout[8] = {}, *P[3] = {};
  int nl = 0, nsp = 0;                  // L1 partials (all images), smoothness partials per image
  SpPackJobs pk = {};
};

static int sp_layout(SpEngine* e, int H, int W, int bs, float* base, size_t* total) {
  size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
  e->H = H; e->W = W; e->bs = bs;
  int o = 0;
  for (int l = 0; l < 10; ++l) {
    SpLayer& L = e->enc[l];
    L.cin = SP_ENC_CH[l]; L.cout = SP_ENC_CH[l + 1];
    L.w_off = o; o += 9 * L.cin * L.cout; L.b_off = o; o += L.cout;
  }
  for (int j = 0; j < 10; ++j) {
    SpLayer& L = e->dec[j];
    L.cin = SP_DEC_IN[j]; L.cout = SP_DEC_OUT[j];
    L.w_off = o; o += 9 * L.cin * L.cout; L.b_off = o; o += L.cout;
  }
  e->n_param = o;
  e->theta = take(o); e->m = take(o); e->v = take(o); e->grad = take(o);
  e->ctr = take(64); e->losses = take(64);
  e->nl = dec_end_lpart_floats(H, W, bs); e->lpart = take(e->nl);
  e->nsp = smooth_loss_blocks(H, W, 64); e->spart = take((size_t)bs * e->nsp);
  const int wsm = wgrad3x3_batched_ws_floats(H, W, bs, 64, 64), ws1 = wgrad3x3_batched_ws_floats(H, W, bs, 32, 1);
  e->wsg = take(wsm > ws1 ? wsm : ws1);
  // packs: Enc 1..9 and Dec 0..7, forward and backward-data, two forms each
  SpPackJobs& J = e->pk;
  J.n = 0; J.total = 0;
  auto job = [&](int src, int cin, int cout, int trans, float** wt, float** wt2) {
    const int n = 9 * cin * cout;
    *wt = take(n); *wt2 = take(n);
    J.j[J.n++] = SpPackJob{*wt, *wt2, src, cin, cout, trans, J.total};
    J.total += n;
  };
  for (int l = 1; l < 10; ++l) {
    SpLayer& L = e->enc[l];                     // Conv2d weight [cout][cin]: forward as is, backward-data transposed + flipped
    job(L.w_off, L.cin, L.cout, 0, &L.fwt, &L.fwt2);
    job(L.w_off, L.cout, L.cin, 1, &L.bwt, &L.bwt2);
  }
  for (int j = 0; j < 8; ++j) {
    SpLayer& L = e->dec[j];                     // ConvTranspose2d weight [nin][nout]: forward transposed + flipped, backward-data as is
    job(L.w_off, L.cin, L.cout, 1, &L.fwt, &L.fwt2);
    job(L.w_off, L.cout, L.cin, 0, &L.bwt, &L.bwt2);
  }
  e->enc[0].fwt = e->enc[0].fwt2 = e->enc[0].bwt = e->enc[0].bwt2 = nullptr;
  for (int j = 8; j < 10; ++j) e->dec[j].fwt = e->dec[j].fwt2 = e->dec[j].bwt = e->dec[j].bwt2 = nullptr;
  const size_t HWp = (size_t)(H + 2) * (W + 2);
  e->is = 64 * HWp; e->i1 = HWp;
  e->xin = take((size_t)bs * H * W);
  e->x0 = take(bs * e->i1); e->r1 = take(bs * e->i1); e->rec = take(bs * e->i1); e->drec = take(bs * e->i1); e->dpre8 = take(bs * e->i1);
  e->act[0] = e->x0;
  for (int l = 1; l <= 10; ++l) e->act[l] = take(bs * e->is);
  for (int j = 0; j < 8; ++j) e->dout[j] = take(bs * e->is);
  for (int k = 0; k < 3; ++k) e->P[k] = take(bs * e->is);
  *total = off;
  return 0;
}

static bool sp_shape_ok(int H, int W, int bs) {
  // conv3x3_mfma_lds stages 128-pixel runs with two halo rows (W <= 139); the weight-gradient rows fit the LDS up to W = 157
  return H >= 2 && W >= 2 && W <= 139 && bs >= 1 && bs <= 4096 && (long long)H * W <= (1ll << 20);
}

// forward (+ losses); train: also the backward, Adam and the repack
static int sp_run(SpEngine* e, hipStream_t s, bool train) {
  const int H = e->H, W = e->W, bs = e->bs;
  const size_t is = e->is, i1 = e->i1;
  const float* th = e->theta;
  CHK(sp_pad(e->xin, e->x0, bs, H, W, s));
  for (int b = 0; b < bs; ++b) CHK(conv3x3_c1(e->x0 + b * i1, th + e->enc[0].w_off, th + e->enc[0].b_off, e->act[1] + b * is, H, W, 32, s));
  for (int l = 1; l < 10; ++l) {
    const SpLayer& L = e->enc[l];
    for (int b = 0; b < bs; ++b)
      CHK(conv3x3_mfma_lds(e->act[l] + b * is, L.fwt, L.fwt2, th + L.b_off, nullptr, e->act[l + 1] + b * is, H, W, L.cin, L.cout, 0, s));
  }
  for (int j = 0; j < 8; ++j) {
    const SpLayer& L = e->dec[j];
    const float* din = j ? e->dout[j - 1] : e->act[10];
    for (int b = 0; b < bs; ++b)
      CHK(conv3x3_mfma_lds(din + b * is, L.fwt, L.fwt2, th + L.b_off, nullptr, e->dout[j] + b * is, H, W, L.cin, L.cout, 0, s));
  }
  const double n_rec = (double)bs * H * W, n_sm = (double)bs * 64 * H * (W - 1);
  CHK(dec_end_fwd(e->dout[7], is, th + e->dec[8].w_off, th + e->dec[8].b_off, th + e->dec[9].w_off, th + e->dec[9].b_off, e->r1, e->rec,
                     e->x0, train ? e->drec : nullptr, (float)(e->w_rec / n_rec), e->lpart, train ? e->ctr : nullptr, e->lr, bs, H, W, s));
  const float coef2 = (float)(2.0 * e->w_smooth / n_sm);
  for (int b = 0; b < bs; ++b) CHK(smooth_loss(e->act[10] + b * is, e->P[2] + b * is, e->spart + (size_t)b * e->nsp, H, W, 64, coef2, s));
  CHK(sp_losses(e->lpart, e->nl, e->spart, bs * e->nsp, n_rec, n_sm, e->w_rec, e->w_smooth, e->losses, s));
  if (!train) return 0;

  // ---- Dec backward
  float* g = e->grad;
  CHK(dec_end_bwd(e->drec, th + e->dec[9].w_off, e->r1, e->dpre8, th + e->dec[8].w_off, e->dout[7], is, e->P[0], bs, H, W, s));
  CHK(wgrad3x3_batched(e->r1, i1, e->drec, i1, bs, H, W, 1, 1, 1, e->wsg, g + e->dec[9].w_off, g + e->dec[9].b_off, s));
  CHK(wgrad3x3_batched(e->dout[7], is, e->dpre8, i1, bs, H, W, 32, 1, 1, e->wsg, g + e->dec[8].w_off, g + e->dec[8].b_off, s));
  float *cur = e->P[0], *oth = e->P[1];
  for (int j = 7; j >= 0; --j) {
    const SpLayer& L = e->dec[j];
    const float* din = j ? e->dout[j - 1] : e->act[10];
    for (int b = 0; b < bs; ++b)                 // d(input) * lrelu'(input): the input is the previous layer's (or Enc's) activation
      CHK(conv3x3_mfma_lds(cur + b * is, L.bwt, L.bwt2, nullptr, din + b * is, oth + b * is, H, W, L.cout, L.cin, 1, s));
    CHK(wgrad3x3_batched(din, is, cur, is, bs, H, W, L.cin, L.cout, 1, e->wsg, g + L.w_off, g + L.b_off, s));
    float* t = cur; cur = oth; oth = t;
  }
  // ---- d(pre-activation of Enc layer 9) = smoothness term (P[2], written by smooth_loss) + Dec's d z * lrelu'(z) (cur)
  CHK(sp_add(e->P[2], cur, (size_t)bs * is, s));
  cur = e->P[2];
  for (int l = 9; l >= 1; --l) {
    const SpLayer& L = e->enc[l];
    for (int b = 0; b < bs; ++b)
      CHK(conv3x3_mfma_lds(cur + b * is, L.bwt, L.bwt2, nullptr, e->act[l] + b * is, oth + b * is, H, W, L.cout, L.cin, 1, s));
    CHK(wgrad3x3_batched(cur, is, e->act[l], is, bs, H, W, L.cout, L.cin, 0, e->wsg, g + L.w_off, g + L.b_off, s));
    float* t = cur; cur = oth; oth = t;
  }
  CHK(wgrad3x3_batched(cur, is, e->x0, i1, bs, H, W, 32, 1, 0, e->wsg, g + e->enc[0].w_off, g + e->enc[0].b_off, s));
  // ---- update
  CHK(sp_adam(e->theta, e->m, e->v, g, e->ctr, e->n_param, s));
  return sp_repack(e->pk, e->theta, s);
}

// ---- the loop level: an epoch of different batches assembled on the device (train_epoch.hpp)
static int sp_epoch_block(const SpEngine* e, const lemo_sptrain_epoch_desc* d, EpochBlock* B) {
  if (!d || !d->data || !d->idx || d->n_clips < 1 || d->n_steps < 1) return LEMO_ERR_ARG;
  if (e->W - 16 < 9 || e->H < 4) return LEMO_ERR_SHAPE;            // reflect padding by (8, 1) needs more than 8 velocity frames, 2 rows
  *B = EpochBlock{d->data, d->idx, nullptr, nullptr, nullptr, d->log, d->n_clips, 0, 0, d->n_steps, LEMO_MASK_NONE, 0};
  return 0;
}

static int sp_epoch_step(SpEngine* e, bool train, hipStream_t s) {
  CHK(sp_assemble(EpochBlock{}, ep_block(e->ctr), 0, e->xin, e->bs, e->H, e->W, s));
  CHK(sp_run(e, s, train));
  return ep_end(ep_block(e->ctr), e->losses, 3, s);
}

}  // namespace lemo

using namespace lemo;

extern "C" {

long long lemo_sptrain_ws_floats(int H, int W, int bs) {
  if (!sp_shape_ok(H, W, bs)) return 0;
  SpEngine e;
  size_t total = 0;
  sp_layout(&e, H, W, bs, nullptr, &total);
  return (long long)total;
}

int lemo_sptrain_n_param(void) {
  SpEngine e;
  size_t total = 0;
  sp_layout(&e, 8, 8, 1, nullptr, &total);
  return e.n_param;
}

void* lemo_sptrain_create(const lemo_sptrain_desc* d) {
  if (!d || !d->ws || !sp_shape_ok(d->H, d->W, d->bs) || !(d->lr > 0.f)) return nullptr;
  if (conv_lds_init() || sp_wgrad_init()) return nullptr;          // LDS opt-ins before any capture
  SpEngine* e = new (std::nothrow) SpEngine();
  if (!e) return nullptr;
  size_t total = 0;
  sp_layout(e, d->H, d->W, d->bs, d->ws, &total);
  if ((long long)total > d->ws_floats) { delete e; return nullptr; }
  e->lr = lr_decimal(d->lr);
  e->w_rec = d->weight_rec; e->w_smooth = d->weight_smooth;
  e->use_graph = d->use_graph;
  return e;
}

void lemo_sptrain_destroy(void* h) {
  SpEngine* e = (SpEngine*)h;
  if (!e) return;
  e->destroy_graphs();
  delete e;
}

int lemo_sptrain_load(void* h, const float* flat, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !flat) return LEMO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_param;
  CHK((int)hipMemcpyAsync(e->theta, flat, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemsetAsync(e->m, 0, sizeof(float) * n, s));          // a fresh optimizer
  CHK((int)hipMemsetAsync(e->v, 0, sizeof(float) * n, s));
  CHK((int)hipMemsetAsync(e->ctr, 0, sizeof(float) * 64, s));
  CHK(sp_repack(e->pk, e->theta, s));
  e->loaded = 1;
  return 0;
}

// n steps on the batch x [bs][H][W] (device); losses (device, may be null) <- {L1 term, smoothness term, weighted sum} of the last step
int lemo_sptrain_step(void* h, const float* x, int n, float* losses, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !x || n < 0) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  CHK((int)hipMemcpyAsync(e->xin, x, sizeof(float) * e->bs * e->H * e->W, hipMemcpyDeviceToDevice, s));
  CHK(replay_or_run(&e->exec, e->use_graph, n, s, [&] { return sp_run(e, s, true); }));
  if (losses) CHK((int)hipMemcpyAsync(losses, e->losses, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
  return 0;
}

// the losses of x under the current parameters, no update; rec (may be null) <- the reconstruction [bs][H + 2][W + 2] (zero border)
int lemo_sptrain_eval(void* h, const float* x, float* losses, float* rec, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !x || !losses) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  CHK((int)hipMemcpyAsync(e->xin, x, sizeof(float) * e->bs * e->H * e->W, hipMemcpyDeviceToDevice, s));
  CHK(sp_run(e, s, false));
  CHK((int)hipMemcpyAsync(losses, e->losses, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
  if (rec) CHK((int)hipMemcpyAsync(rec, e->rec, sizeof(float) * e->bs * e->i1, hipMemcpyDeviceToDevice, s));
  return 0;
}

int lemo_sptrain_params(void* h, float* flat_out, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !flat_out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  return (int)hipMemcpyAsync(flat_out, e->theta, sizeof(float) * e->n_param, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int lemo_sptrain_grads(void* h, float* flat_out, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !flat_out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  return (int)hipMemcpyAsync(flat_out, e->grad, sizeof(float) * e->n_param, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int lemo_sptrain_epoch(void* h, const lemo_sptrain_epoch_desc* d, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !d || !d->log) return LEMO_ERR_ARG;
  EpochBlock B;
  CHK(sp_epoch_block(e, d, &B));
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const bool train = d->train != 0;
  CHK(ep_begin(B, ep_block(e->ctr), s));
  return replay_or_run(&e->exec_ep[train], e->use_graph, d->n_steps, s, [&] { return sp_epoch_step(e, train, s); });
}

int lemo_sptrain_batch(void* h, const lemo_sptrain_epoch_desc* d, int step, float* x, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !x) return LEMO_ERR_ARG;
  EpochBlock B;
  CHK(sp_epoch_block(e, d, &B));
  if (step < 0 || step >= d->n_steps) return LEMO_ERR_ARG;
  return sp_assemble(B, nullptr, step, x, e->bs, e->H, e->W, (hipStream_t)stream);
}

long long lemo_sptrain_state_floats(void) { return 3ll * lemo_sptrain_n_param() + 2; }

int lemo_sptrain_state_save(void* h, float* out, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !out) return LEMO_ERR_ARG;
  if (!e->loaded) return LEMO_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_param;
  CHK((int)hipMemcpyAsync(out, e->theta, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemcpyAsync(out + n, e->m, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemcpyAsync(out + 2 * n, e->v, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  return train_step_counter(e->ctr, out + 3 * n, true, s);
}

int lemo_sptrain_state_load(void* h, const float* in, void* stream) {
  SpEngine* e = (SpEngine*)h;
  if (!e || !in) return LEMO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_param;
  CHK((int)hipMemcpyAsync(e->theta, in, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemcpyAsync(e->m, in + n, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemcpyAsync(e->v, in + 2 * n, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  CHK((int)hipMemsetAsync(e->ctr, 0, sizeof(float) * 64, s));
  CHK(train_step_counter(e->ctr, const_cast<float*>(in) + 3 * n, false, s));
  CHK(sp_repack(e->pk, e->theta, s));
  e->loaded = 1;
  return 0;
}

long long lemo_wgrad3x3_batched_ws_floats(int H, int W, int bs, int ca, int cb) {
  if (bs < 1 || H < 1 || W < 1) return 0;
  return wgrad3x3_batched_ws_floats(H, W, bs, ca, cb);
}

int lemo_wgrad3x3_batched(const float* A, long long a_stride, const float* B, long long b_stride, int bs, int H, int W, int ca, int cb,
                          int bias_b, float* ws, float* gw, float* gb, void* stream) {
  if (a_stride < 0 || b_stride < 0) return LEMO_ERR_ARG;
  return wgrad3x3_batched(A, (size_t)a_stride, B, (size_t)b_stride, bs, H, W, ca, cb, bias_b, ws, gw, gb, (hipStream_t)stream);
}

int lemo_dec_end_fwd(const float* u, long long u_stride, const float* w8, const float* b8, const float* w9, const float* b9, float* r1,
                     float* rec, int bs, int H, int W, void* stream) {
  if (u_stride < 0) return LEMO_ERR_ARG;
  return dec_end_fwd(u, (size_t)u_stride, w8, b8, w9, b9, r1, rec, nullptr, nullptr, 0.f, nullptr, nullptr, 0.0, bs, H, W, (hipStream_t)stream);
}

}  // extern "C"
