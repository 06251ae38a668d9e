// The infilling autoencoder's network, written once for its two engines -- the finetune engine (ae_engine.hip: K clips, K parameter
// sets) and the batch trainer (ae_train_engine.hip: one parameter set over bs images).  Shared here: the convolution launcher's
// interface, the layer table with every parameter / partial offset (ae_net_layers), the per-image workspace region and its wiring
// (ae_net_carve_image), the forward and backward-data launch chains (ae_net_forward, ae_net_backward_data), the weight-gradient job
// table (ae_wgrad_jobs), and the optimiser's and the packing launches with their arguments (ae_adam_args, ae_pack_args).  An engine
// keeps what is its own: the shared / optimiser buffers around the per-image region, its loss, its weight-gradient kernel, and how a
// convolution of the chains is launched (clip count, weight stride, split-f16 scale slots).
#pragma once
#include "kernels.hpp"
#include "engine_host.hpp"

namespace lemo {

// A pixel (y, x) of the H x W grid the launch enumerates sits at padded pixel ((s y + 1) Wp + s x + 1) of a buffer with
// row pitch Wp and stride s (1: plain CG8P of an H x W image; 2: the even pixels of a twice finer image = zero-stuffing
// geometry).  Taps always address neighbouring pixels of the INPUT buffer.
struct AeGeo { int H, W; int in_Wp, in_HWp, in_s; int out_Wp, out_HWp, out_s; int aux_Wp, aux_HWp, aux_s; };
static inline AeGeo geo_plain(int H, int W) { const int Wp = W + 2, HWp = (H + 2) * Wp; return AeGeo{H, W, Wp, HWp, 1, Wp, HWp, 1, Wp, HWp, 1}; }

struct AeF16;
// wcs: the parameter stride between clips; AE_WCS_CLIP = the clip stride cs (per-clip parameters), 0 = one shared parameter set
#define AE_WCS_CLIP ((size_t)-1)
int ae_conv(const float* in, const float* wt, const float* bias, const float* aux, float* out, const AeGeo& g, int cin, int cout,
            int epi, hipStream_t s, int force_mt = 0, int force_pt = 0, int force_ks = 0, int nclip = 1, size_t cs = 0,
            const AeF16* f16 = nullptr, size_t wcs = AE_WCS_CLIP);

static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

#define AE_NLAYER 20
#define AE_SLAB 576               // padded pixels per slab, at most (a layer's slabs are equal parts: ae_slabs)
static const int AE_ENC[5][2] = {{4, 32}, {32, 64}, {64, 128}, {128, 256}, {256, 256}};      // models/AE.py:81-91, in_channel = 4
static const int AE_DEC[5][2] = {{256, 256}, {256, 128}, {128, 64}, {64, 32}, {32, 1}};

struct AeLayer { int cin, cout, cin_pad, cout_pad, deconv, level, w_off, b_off, wb_off, flat_w, flat_b, nslab, slab_len; size_t part_off, dbp_off; };

// slabs of padded interior pixels for the weight gradients: equal parts of at most AE_SLAB pixels, a multiple of 32 long (27 x 19
// = 513 padded pixels is ONE slab, not 512 + 1)
// `scale` (round 5, measured and NOT adopted): with k clips side by side the launch has k x the waves, so a clip's slabs could be k x
// longer for the same number of waves in flight (fewer partial tiles written by the weight-gradient launch and read back by the
// optimiser launch).  8 clips per engine, ms per clip: x1 16.40, x2 16.69, x4 17.24, x8 18.07, x16 20.51; 16 clips: x1 15.43, x4 15.76,
// x8 16.32 (profiles/r05_ab_ae_slab_scale.txt) -- the launch wants MANY SHORT waves (its cost is the spread between a level-0 wave
// and a level-4 one, not the 40 MB of partials per clip), so the scale stays 1; LEMO_AE_SLAB_SCALE keeps the switch
static inline int ae_slabs(int H, int W, int* len, int scale = 1) {
  const int cap = AE_SLAB * (scale < 1 ? 1 : scale);
  const int n_px = H * (W + 2), n = (n_px + cap - 1) / cap;
  *len = ((n_px + n - 1) / n + 31) / 32 * 32;
  return (n_px + *len - 1) / *len;
}

static inline int pad8(int c) { return (c + 7) / 8 * 8; }
static inline int pad32(int c) { return (c + 31) / 32 * 32; }
static inline size_t cg8p_floats(int C, int H, int W) { return (size_t)(C / 8 > 0 ? C / 8 : 1) * (H + 2) * (W + 2) * 8; }

// every buffer is wrapped in AE_GUARD zeroed floats that nothing writes: the weight-gradient kernel's operand windows may
// reach up to 17 pixels (136 floats) past either end of a CG8P buffer, at positions whose products are multiplied by zero
#define AE_GUARD 256
struct Bump {
  float* base; size_t off = 0;
  float* take(size_t n) { float* p = base ? base + off + AE_GUARD : nullptr; off += (n + 2 * AE_GUARD + 63) / 64 * 64; return p; }
};

// optimizer: slab reduction + Adam + backward pack, one launch over the packed parameter vector (ae_engine.hip: ae_adam_kernel)
struct AeAdamLayer { const float* partial; const float* dbp; int nslab, w_off, b_off, wb_off, cin_lg /*log2(cin_pad/8)*/, cout_lg, cin, cout; };
struct AeAdamArgs {
  AeAdamLayer L[AE_NLAYER];
  float* theta; float* m; float* v; float* wb; const float* ctr;    // ctr: [1] = -lr / (1 - b1^t), [2] = sqrt(1 - b2^t) (floats)
  float* amax;                                                      // the step's tensor maxima: slots 0 .. AE_SLOT_DYN - 1 zeroed here for the next step
  int n_w, n_all; float lr;
  size_t cs;                                                        // clip stride (clip = blockIdx.y)
};
int ae_adam_launch(const AeAdamArgs& A, int nclip, hipStream_t s);

// the model's own tensors (state_dict order) <-> theta (+ the backward pack); unpack: theta -> flat
struct AePackLayer { int w_off, wb_off, b_off, flat_w, flat_b, cin_lg, cout_lg, cin, cout, deconv; };
struct AePackArgs { AePackLayer L[AE_NLAYER]; int n_w, n_all; };
int ae_pack_launch(const AePackArgs& A, bool unpack, const float* src, float* dst, float* wb, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------------
// the network: 5 encoder blocks (conv, conv, max pool), zero stuffing, 5 decoder blocks (two transposed convs as convs of the stuffed input)
// ---------------------------------------------------------------------------------------------------------------------
struct AeNet {
  int H[6], W[6];              // level sizes: level k + 1 = level k pooled 3 x 3, stride 2
  AeLayer L[AE_NLAYER];
  int n_w = 0, n_b = 0, n_wb = 0, n_flat = 0;
  // image (clip) 0's buffers; image c's are the engine's stride further
  float* x8 = nullptr;
  float* act[AE_NLAYER];       // output of layer i (decoder blocks 0..3: their second layer's output lives stuffed in S[b + 1])
  float* xin[AE_NLAYER];       // input of layer i
  float* dp[AE_NLAYER];        // d(pre-activation) of layer i
  float *P[5], *dP[5], *S[5];
  unsigned char* idx[5];
};

// level sizes, layer rows and every offset.  slab_scale: ae_slabs; groups: partial tiles per pixel slab (the trainer's image groups).
// Returns the floats of all weight-gradient partials and of all bias-gradient partials.
struct AePartials { size_t part, dbp; };
static inline AePartials ae_net_layers(AeNet& n, int H0, int W0, int slab_scale, int groups) {
  n.H[0] = H0; n.W[0] = W0;
  for (int k = 0; k < 5; ++k) { n.H[k + 1] = (n.H[k] - 1) / 2 + 1; n.W[k + 1] = (n.W[k] - 1) / 2 + 1; }
  int i = 0;
  for (int b = 0; b < 5; ++b) {
    const int ci = AE_ENC[b][0], co = AE_ENC[b][1];
    n.L[i++] = AeLayer{ci, co, pad8(ci), pad32(co), 0, b};
    n.L[i++] = AeLayer{co, co, pad32(co), pad32(co), 0, b};
  }
  for (int b = 0; b < 5; ++b) {
    const int ci = AE_DEC[b][0], co = AE_DEC[b][1];
    n.L[i++] = AeLayer{ci, co, pad32(ci), pad32(co), 1, 4 - b};
    n.L[i++] = AeLayer{co, co, pad32(co), pad32(co), 1, 4 - b};
  }
  int w = 0, wbo = 0, flat = 0, b = 0;
  AePartials t{0, 0};
  for (i = 0; i < AE_NLAYER; ++i) {
    AeLayer& l = n.L[i];
    l.w_off = w; w += 9 * l.cin_pad * l.cout_pad;
    l.wb_off = i == 0 ? -1 : wbo; if (i) wbo += 9 * l.cin_pad * l.cout_pad;      // the first layer needs no backward-data
    l.flat_w = flat; flat += 9 * l.cin * l.cout;
    l.flat_b = flat; flat += l.cout;
    l.b_off = b; b += l.cout_pad;
    l.nslab = ae_slabs(n.H[l.level], n.W[l.level], &l.slab_len, slab_scale);
    l.part_off = t.part; t.part += (size_t)groups * l.nslab * 9 * l.cin_pad * l.cout_pad;
    l.dbp_off = t.dbp; t.dbp += (size_t)groups * l.nslab * 2 * l.cout_pad;
  }
  n.n_w = w; n.n_b = b; n.n_wb = wbo; n.n_flat = flat;
  return t;
}

// one image's region of the workspace, and which buffer every layer reads
static inline void ae_net_carve_image(AeNet& n, Bump& B) {
  n.x8 = B.take(cg8p_floats(8, n.H[0], n.W[0]));
  for (int bk = 0; bk < 5; ++bk) {
    const int lv = bk, i0 = 2 * bk, i2 = 2 * bk + 1;
    n.act[i0] = B.take(cg8p_floats(n.L[i0].cout_pad, n.H[lv], n.W[lv]));
    n.act[i2] = B.take(cg8p_floats(n.L[i2].cout_pad, n.H[lv], n.W[lv]));
    n.P[bk] = B.take(cg8p_floats(n.L[i2].cout_pad, n.H[lv + 1], n.W[lv + 1]));
    n.dP[bk] = B.take(cg8p_floats(n.L[i2].cout_pad, n.H[lv + 1], n.W[lv + 1]));
    n.idx[bk] = reinterpret_cast<unsigned char*>(B.take(((size_t)n.L[i2].cout_pad * n.H[lv + 1] * n.W[lv + 1] + 3) / 4));
    n.xin[i0] = bk == 0 ? n.x8 : n.P[bk - 1];
    n.xin[i2] = n.act[i0];
  }
  for (int bk = 0; bk < 5; ++bk) n.S[bk] = B.take(cg8p_floats(n.L[10 + 2 * bk].cin_pad, n.H[4 - bk], n.W[4 - bk]));
  for (int bk = 0; bk < 5; ++bk) {
    const int lv = 4 - bk, i1 = 10 + 2 * bk, i2 = 11 + 2 * bk;
    n.act[i1] = B.take(cg8p_floats(n.L[i1].cout_pad, n.H[lv], n.W[lv]));
    n.act[i2] = bk < 4 ? n.S[bk + 1] : B.take(cg8p_floats(n.L[i2].cout_pad, n.H[lv], n.W[lv]));
    n.xin[i1] = n.S[bk];
    n.xin[i2] = n.act[i1];
  }
  for (int i = 0; i < AE_NLAYER; ++i) n.dp[i] = B.take(cg8p_floats(n.L[i].cout_pad, n.H[n.L[i].level], n.W[n.L[i].level]));
}

// slots of the finetune engine's amax block (tensor maxima the split-f16 convolutions scale by).  0 .. AE_SLOT_DYN - 1 are rewritten
// every step (zeroed by the optimiser launch and at load)
#define AE_SLOT_ACT(i) (i)                /* max |output of layer i| (forward) */
#define AE_SLOT_DP(i) (20 + (i))          /* max |d(pre-activation) of layer i| where a convolution wrote it */
#define AE_SLOT_DPOOL(b) (40 + (b))       /* max |d(pooled output of encoder block b)| */
#define AE_SLOT_DYN 45
#define AE_SLOT_X8 45                     /* the clip image */
#define AE_SLOT_LOSS 46                   /* max (mask / count): the loss gradient is +-1 x that */
#define AE_SLOT_W(i) (48 + (i))           /* max |weights of layer i| (forward and backward pack hold the same values) */
#define AE_SLOT_SCRATCH 70
#define AE_NSLOT 128

// The two chains launch their convolutions through the engine's `conv(site, in, wt, bias, aux, out, geo, cin, cout, epi)`, which adds
// what is the engine's own (clip count and stride, weight stride, stream, the AeF16 of `site` or none).  site: the scale slots of a
// split-f16 launch -- the input's maximum (x fac: a bound), the weights of layer `w`, the slot that receives the output's maximum.
struct AeConvSite { int in; float fac; int w; int out; };
// the launches that are no convolution take the images per launch, their stride and the stream as they are
struct AeBatch { int n; size_t cs; hipStream_t s; };

template <class Conv>
static int ae_net_forward(const AeNet& n, const float* theta, const AeBatch& bt, Conv&& conv) {
  // (pooling and zero stuffing keep the maximum: the pooled / stuffed inputs scale by their source's slot)
  const auto layer = [&](int i, const AeGeo& g, int epi) {
    const AeLayer& l = n.L[i];
    return conv(AeConvSite{i == 0 ? AE_SLOT_X8 : AE_SLOT_ACT(i - 1), 1.f, i, AE_SLOT_ACT(i)}, n.xin[i], theta + l.w_off,
                theta + n.n_w + l.b_off, nullptr, n.act[i], g, l.cin_pad, l.cout_pad, epi);
  };
  for (int b = 0; b < 5; ++b) {
    const int H = n.H[b], W = n.W[b], i0 = 2 * b, i2 = 2 * b + 1;
    const AeGeo g = geo_plain(H, W);
    CHK(layer(i0, g, 0));
    CHK(layer(i2, g, 0));
    CHK(maxpool3s2_fwd(n.act[i2], H, W, n.P[b], n.idx[b], n.L[i2].cout_pad, bt.s, bt.n, bt.cs));
  }
  CHK(stuff2_fwd(n.P[4], n.H[5], n.W[5], n.S[0], n.H[4], n.W[4], n.L[10].cin_pad, bt.s, bt.n, bt.cs));
  for (int b = 0; b < 5; ++b) {
    const int lv = 4 - b, H = n.H[lv], W = n.W[lv], i1 = 10 + 2 * b, i2 = 11 + 2 * b;
    AeGeo g = geo_plain(H, W);
    CHK(layer(i1, g, 0));
    if (b < 4) {       // straight into the stuffed input of the next block: pixel (y, x) -> (2y, 2x) of the next finer level
      g.out_Wp = n.W[lv - 1] + 2; g.out_HWp = (n.H[lv - 1] + 2) * g.out_Wp; g.out_s = 2;
    }
    CHK(layer(i2, g, b < 4 ? 0 : 2));
  }
  return 0;
}

// d(pre-activation) of every layer from dp[19] (the loss adjoint), last layer first.  wb: the backward pack
template <class Conv>
static int ae_net_backward_data(const AeNet& n, const float* wb, const float* zero_bias, const AeBatch& bt, Conv&& conv) {
  // layer i's backward-data convolution: times lrelu'(aux) of the layer below (epilogue 1), or the plain sum where the tensor below
  // has no activation (a pooled map, the latent: epilogue 2 with a zero bias)
  const auto back = [&](int i, int in_slot, float fac, int out_slot, const float* aux, float* out, const AeGeo& g) {
    const AeLayer& l = n.L[i];
    return conv(AeConvSite{in_slot, fac, i, out_slot}, n.dp[i], wb + l.wb_off, aux ? nullptr : zero_bias, aux, out, g, l.cout_pad,
                l.cin_pad, aux ? 1 : 2);
  };
  // ---- decoder, last block first
  for (int b = 4; b >= 0; --b) {
    const int lv = 4 - b, H = n.H[lv], W = n.W[lv], i1 = 10 + 2 * b, i2 = 11 + 2 * b;
    CHK(back(i2, i2 == 19 ? AE_SLOT_LOSS : AE_SLOT_DP(i2), 1.f, AE_SLOT_DP(i1), n.act[i1], n.dp[i1], geo_plain(H, W)));
    // adjoint of (stuffing, transposed conv): only the even pixels of d(stuffed input) exist downstream -> enumerate the
    // coarse grid, centre taps at (2i, 2j); times lrelu' of the previous block's output (read where it lives: stuffed in S[b])
    AeGeo gs = geo_plain(n.H[lv + 1], n.W[lv + 1]);
    gs.in_Wp = W + 2; gs.in_HWp = (H + 2) * (W + 2); gs.in_s = 2;
    gs.aux_Wp = gs.in_Wp; gs.aux_HWp = gs.in_HWp; gs.aux_s = 2;
    if (b > 0) CHK(back(i1, AE_SLOT_DP(i1), 1.f, AE_SLOT_DP(i1 - 1), n.S[b], n.dp[i1 - 1], gs));
    else       CHK(back(i1, AE_SLOT_DP(i1), 1.f, AE_SLOT_DPOOL(4), nullptr, n.dP[4], gs));        // the latent has no activation
  }
  // ---- encoder, last block first
  for (int b = 4; b >= 0; --b) {
    const int H = n.H[b], W = n.W[b], i0 = 2 * b, i2 = 2 * b + 1;
    const AeGeo g = geo_plain(H, W);
    CHK(maxpool3s2_bwd(n.dP[b], n.idx[b], n.act[i2], n.dp[i2], H, W, n.L[i2].cout_pad, bt.s, bt.n, bt.cs));
    // (the max-pool adjoint adds at most four window gradients into one pixel, times lrelu' <= 1: dp[i2] is bounded by 4 x the pooled gradient's maximum)
    CHK(back(i2, AE_SLOT_DPOOL(b), 4.f, AE_SLOT_DP(i0), n.act[i0], n.dp[i0], g));
    if (b > 0) CHK(back(i0, AE_SLOT_DP(i0), 1.f, AE_SLOT_DPOOL(b - 1), nullptr, n.dP[b - 1], g));
  }
  return 0;
}

// One layer's weight- and bias-gradient work: a wave per (slab, co tile, ci tile, kernel row); image (clip) 0's operands.
// dbp: [nslab][2][cout] bias-gradient partials (pixel parity kept apart); the trainer's partial / dbp carry a leading [group]
struct AeWgradJob {
  const float* dy; const float* x; float* partial; float* dbp;
  int H, W; int cin, cout, nslab, slab_len, nwave;
};
// the jobs in the order the launch wants them DISPATCHED: the big images' layers (long waves) first, so that the launch does not end
// on a few long waves; first[k]: job k's first block, first[n]: the grid
struct AeWgradCount { int n, nb; };
static inline AeWgradCount ae_wgrad_jobs(const AeNet& net, float* part, float* dbp, AeWgradJob* j, int* first) {
  int nb = 0, n = 0;
  for (int lv = 0; lv < 5; ++lv)
    for (int i = 0; i < AE_NLAYER; ++i) {
      const AeLayer& l = net.L[i];
      if (l.level != lv) continue;
      AeWgradJob& q = j[n];
      q.dy = net.dp[i]; q.x = net.xin[i]; q.partial = part + l.part_off; q.dbp = dbp + l.dbp_off;
      q.H = net.H[l.level]; q.W = net.W[l.level];
      q.cin = l.cin_pad; q.cout = l.cout_pad; q.nslab = l.nslab; q.slab_len = l.slab_len;
      q.nwave = 3 * l.nslab * (l.cout_pad / 32) * ((l.cin_pad + 31) / 32);
      first[n++] = nb;
      nb += q.nwave;
    }
  first[n] = nb;
  return AeWgradCount{n, nb};
}

// the optimiser launch's arguments; nslab_factor: partial tiles per pixel slab (ae_net_layers' groups); cs: the clips' stride (0: one clip)
static inline AeAdamArgs ae_adam_args(const AeNet& n, const float* part, const float* dbp, int nslab_factor, float* theta, float* m,
                                      float* v, float* wb, const float* ctr, float* amax, float lr, size_t cs) {
  AeAdamArgs A;
  A.theta = theta; A.m = m; A.v = v; A.wb = wb; A.ctr = ctr; A.amax = amax; A.lr = lr; A.cs = cs;
  for (int i = 0; i < AE_NLAYER; ++i) {
    const AeLayer& l = n.L[i];
    A.L[i] = AeAdamLayer{part + l.part_off, dbp + l.dbp_off, nslab_factor * l.nslab, l.w_off, l.b_off, l.wb_off,
                         ilog2(l.cin_pad / 8), ilog2(l.cout_pad), l.cin, l.cout};
  }
  A.n_w = n.n_w; A.n_all = n.n_w + n.n_b;
  return A;
}

static inline AePackArgs ae_pack_args(const AeNet& n) {
  AePackArgs A;
  for (int i = 0; i < AE_NLAYER; ++i) {
    const AeLayer& l = n.L[i];
    A.L[i] = AePackLayer{l.w_off, l.wb_off, l.b_off, l.flat_w, l.flat_b, ilog2(l.cin_pad / 8), ilog2(l.cout_pad), l.cin, l.cout, l.deconv};
  }
  A.n_w = n.n_w; A.n_all = n.n_w + n.n_b;
  return A;
}

}  // namespace lemo
