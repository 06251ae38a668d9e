// Pieces of the infilling autoencoder's step engine (ae_engine.hip) that its batched trainer (ae_train_engine.hip) shares: the
// convolution launcher, the layer table and parameter layout, the workspace carving, the optimiser and packing launches.
#pragma once
#include "kernels.hpp"

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

}  // namespace lemo
