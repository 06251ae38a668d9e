// The encoder's turn from forward to backward in ONE launch ("the turn", conv variant 9's step schedule): layer 9 forward
// (64 -> 64, models/AE_sep.py:11-30), the latent smoothness loss and its gradient (opt_amass_temp.py:390-391, smooth_loss_body in
// loss_device.hpp), and layer 9's backward-data, on 2-D tiles with everything between the two convolutions kept in LDS.
//
// Why: d(pre-act 10) = coef2 * (3-tap stencil of z along x) * lrelu'(z) is a LOCAL function of z = act[10], so the backward-data of
// layer 9 can follow its forward in the same workgroup.  This replaces three launches of the step (layer 9 forward as an unpaired
// split launch, the fit_losses launch, layer 3's backward-data as an unpaired split launch: the 7 + 7 layer applications of the
// 64 -> 64 part then all run in pairs or here).  A workgroup owns a TH x TW = 12 x 12 output tile of d(pre-act 9):
//   in    act[9] on (TH+4) x (TW+6) = 16 x 18 = 288 px, staged once as two fp16 pieces, [group 8][piece 2][px][8 x f16] = 72 KB
//   z     layer 9 forward on (TH+2) x (TW+4) = 14 x 16 = 224 px = 7 MFMA N-tiles (2 rows x 16 columns, the pair's layer-1 geometry:
//         the stencil needs z one column beyond every d(pre-act 10) value); bias + LeakyReLU; fp32 copy in LDS for the stencil; the
//         owned 12 x 12 interior is written to act[10] (the tensor the forward-only path publishes)
//   dpre  d(pre-act 10) on (TH+2) x (TW+2) = 14 x 14 px, zero outside the image (layer 9's backward zero padding), split with one
//         power-of-two scale for the tile into planes of row pitch 20 (70 KB)
//   out   d(pre-act 9) = conv^T(dpre, w9) * lrelu'(act[9]) on the 144 owned pixels, packed into 5 N-tiles (16 lanes idle)
// ceil(245 / 12) x ceil(134 / 12) = 21 x 12 = 252 workgroups of 8 waves: one per CU, one round.  Matrix work 12 N-tiles x 2 M-tiles x
// 36 k-steps x 3 products against the pair's 11.  Halo z values (the ring outside the owned tile) are recomputed here under THIS
// workgroup's input scale, as the forward pair recomputes its mid tile: they agree with the neighbour's owned values to fp32 rounding,
// not bitwise.  Owned d(pre-act 10) values are computed from the z this workgroup writes, in smooth_loss_body's order: bit-identical
// to that body applied to the published act[10].
//
// Arithmetic and waves as in the pair (conv_pair.hpp, conv_f16.hpp): w = ng + 2 ch + 4 kh; both convolutions use N-tile group
// g = ng ^ kh so that the two waves of a SIMD (w, w + 4) carry 4 + 3 (z) and 3 + 2 (out) tiles; K halves summed through LDS in the
// fixed order kh 0 + kh 1.  Loss: the sum over owned pixels x <= W - 2 and all channels of (z[x+1] - z[x])^2, one f32 sum per
// workgroup added in f64 to acc + (blockIdx & 31) * 16 (smooth_loss_body's convention; loss_finalize reads it unchanged).
//
// Frame roles (engine use, FrameLoss): nfb extra workgroups after the tiles compute vertex_loss_row16 for 32 frames each (4 per wave),
// so that the per-frame losses need no launch of their own; with 252 tiles and B = 119 that is 256 workgroups, one per CU.
#include "conv_common.hpp"
#include "conv_f16.hpp"
#include "conv_pair.hpp"
#include "loss_device.hpp"

namespace lemo {

constexpr int TT_TH = 12, TT_TW = 12;
constexpr int TT_INW = TT_TW + 6, TT_INH = TT_TH + 4, TT_NIN = TT_INW * TT_INH;        // 18 x 16 = 288
constexpr int TT_ZW = TT_TW + 4, TT_ZH = TT_TH + 2, TT_NZ = TT_ZW * TT_ZH;             // 16 x 14 = 224 = 7 N-tiles
constexpr int TT_DW = TT_TW + 2, TT_DH = TT_TH + 2, TT_ND = TT_DW * TT_DH;             // 14 x 14 = 196
constexpr int TT_DP = 20, TT_NDP = TT_DP * TT_DH;                                      // dpre planes: row pitch 20 (conflict-free B reads), 280 slots
constexpr int TT_NOUT = TT_TH * TT_TW;                                                 // 144 outputs in 5 N-tiles
constexpr int TT_PL_IN = TT_NIN * 16, TT_GRP_IN = 2 * TT_PL_IN;
constexpr int TT_PL_D = TT_NDP * 16, TT_GRP_D = 2 * TT_PL_D;
constexpr int TT_D_OFF = 8 * TT_GRP_IN;                                                // 73,728
constexpr int TT_WMAX_OFF = TT_D_OFF + 8 * TT_GRP_D;                                   // 145,408
constexpr int TT_SMEM = TT_WMAX_OFF + 4 * 8 * 4;                                       // 145,536
constexpr int TT_NSLOT = 5;                                                            // staging slots per thread and phase
constexpr int TT_NITEM = 8 * TT_ND * 2, TT_KITEM = (TT_NITEM + 511) / 512;              // stencil items (float4s): 3136, 7 per thread
constexpr int TT_FRAMES = 32;                                                          // frames per frame-role workgroup (16 lanes each)
static_assert(TT_ZW == 16 && TT_NZ == 7 * 32 && TT_INW == 18, "z N-tiles = 2 rows x 16 columns on the input grid of row pitch 18");
static_assert(4 * 2 * TT_NIN <= TT_NSLOT * 512 && TT_NOUT <= 5 * 32, "staging slots / output tiles");
static_assert(8 * 8 * 256 * 4 <= TT_D_OFF && 8 * 6 * 256 * 4 <= TT_D_OFF, "the K-half exchanges fit the dead input planes");
static_assert(8 * TT_NZ * 8 * 4 <= 8 * TT_GRP_D, "the fp32 z tile fits the (not yet written) dpre planes");

// out N-tile lane -> owned pixel oy * 12 + ox (+256: idle lane, reads that pixel's slot and stores nothing).  With row pitch 20 the
// slot (oy + 1) * 20 + ox + 1 takes every residue mod 16 exactly 9 times over the 144 pixels; the table gives each ds_read_b128 lane
// group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}) 16 distinct residues: conflict-free B reads for every tap (cf. cp_lane_col).
__constant__ unsigned short tt_pix[160] = {
    0,   1,   2,   3,   12,  13,  14,  15,  16,  17,  18,  19,  4,   5,   6,   7,   28,  29,  30,  31,  8,   9,   10,  11,
    20,  21,  22,  23,  32,  33,  34,  35,  24,  25,  26,  27,  48,  49,  50,  51,  52,  53,  54,  55,  36,  37,  38,  39,
    56,  57,  58,  59,  40,  41,  42,  43,  44,  45,  46,  47,  68,  69,  70,  71,  60,  61,  62,  63,  72,  73,  74,  75,
    84,  85,  86,  87,  64,  65,  66,  67,  88,  89,  90,  91,  76,  77,  78,  79,  80,  81,  82,  83,  92,  93,  94,  95,
    96,  97,  98,  99,  108, 109, 110, 111, 112, 113, 114, 115, 100, 101, 102, 103, 124, 125, 126, 127, 104, 105, 106, 107,
    116, 117, 118, 119, 128, 129, 130, 131, 120, 121, 122, 123, 256, 257, 258, 259, 260, 261, 262, 263, 132, 133, 134, 135,
    264, 265, 266, 267, 136, 137, 138, 139, 140, 141, 142, 143, 276, 277, 278, 279};

struct TurnArgs {
  const float* in;                 // act[9], CG8P 64 channels (also the backward epilogue's lrelu' operand)
  const uint4* wf;                 // layer 9 forward split-f16 pack, its inverse host scale
  const uint4* wb;                 // layer 9 backward-data split-f16 pack
  const float* bias;
  float* z;                        // act[10]: the owned interior is written
  float* out;                      // d(pre-act 9)
  float* dpre;                     // optional (tests): d(pre-act 10) of the owned pixels, CG8P
  double* acc;                     // smoothness sum of squares: acc + (blockIdx & 31) * 16
  float winvf, winvb, coef2;
  int H, W, ntx, ntiles;
  FrameLoss fl;                    // frame roles (nfb == 0: none)
  int nfb;
  unsigned long long* dbg;
};

// layer 9 forward for a wave that carries NT (4 | 3) z N-tiles starting at tile T0 (group g), the input staging's second phase riding
// in its first k-chunk as in the pair.  Leaves the kept quads' z values in zv (bias + LeakyReLU, zero outside the image), their fp32
// copy in the z tile, and what the final act[10] store needs.
struct TurnZ { float4 v[8]; int po[2]; bool own[2]; };

template <int NT>
__device__ __forceinline__ void turn_forward(const TurnArgs& a, unsigned char* smem, float* smem_f, float* wmax, int y0, int x0, int g, int ch,
                                             int kh, int lane, int wave, uint4 (&ra)[CP_RA][2], float (&sc)[2], float (&sci)[2],
                                             float4 (&stB)[TT_NSLOT], const int (&dstB)[TT_NSLOT], TurnZ& zs) {
  const int j = lane & 31, h = lane >> 5, T0 = g ? 4 : 0;
  const int H = a.H, W = a.W, Wp = W + 2;
  int li[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) li[nt] = (2 * (T0 + nt) + (j >> 4) + 1) * TT_INW + cp_lane_col(j) + 1;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
  pair_kloop<NT, TT_GRP_IN, TT_PL_IN, TT_INW>(
      acc, ra, a.wf, smem, li, kh, ch, lane,
      [&](int cc, int tap) {
        if (cc != 0) return;
        if (tap == 0) {
          float m = 0.f;
#pragma unroll
          for (int k = 0; k < TT_NSLOT; ++k) m = absmax4(stB[k], m);
          m = wave_max(m);
          if (lane == 0) wmax[8 + wave] = m;
        }
        if (tap == 1) {
          __syncthreads();
          float mm = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) mm = fmaxf(mm, wmax[8 + i]);
          f16_scale_after(mm, sc[0], sc[1], sci[1]);
        }
#pragma unroll
        for (int k = 0; k < TT_NSLOT; ++k) {
          if (2 + (7 * k) / TT_NSLOT != tap) continue;
          uint2 s0, s1;
          split2x4(stB[k], sc[1], s0, s1);
          *reinterpret_cast<uint2*>(smem + 2 * TT_GRP_IN + dstB[k]) = s0;
          *reinterpret_cast<uint2*>(smem + 2 * TT_GRP_IN + dstB[k] + TT_PL_IN) = s1;
        }
      },
      [&](int cc) {
        __syncthreads();
        if (cc == 0) {
          const float f = sc[1] * sci[0];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] *= f;
        }
      });
  {
    const float f = sci[1] * a.winvf;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] *= f;
  }
  typedef PairSplit<NT> S;
  const int KHu = __builtin_amdgcn_readfirstlane(kh);
  // the two tiles whose quads this half finishes: slot 0 = tile KH of the group, slot 1 = tile 2 + KH (NT 4) | 2 (NT 3)
  int zp[2];
  bool inimg[2];
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int t = T0 + (sl == 0 ? KHu : (NT == 4 ? 2 + KHu : 2));
    const int zr = 2 * t + (j >> 4), zc = cp_lane_col(j);
    const int y = y0 - 1 + zr, x = x0 - 2 + zc;
    zp[sl] = zr * TT_ZW + zc;
    inimg[sl] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    zs.own[sl] = inimg[sl] && zr >= 1 && zr <= TT_TH && zc >= 2 && zc <= TT_TW + 1;
    const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y), xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
    zs.po[sl] = (yc + 1) * Wp + (xc + 1);
  }
  float4 eo[S::NQ];
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int q = KHu ? S::keep_quad(1, i) : S::keep_quad(0, i);
    eo[i] = ld4(a.bias + ch * 32 + q * 8 + 4 * h);
  }
  float4 v[S::NQ];
  {
    float* red = smem_f + ((g * 2 + ch) * 2) * 2048 + lane * 4;      // the input planes are dead (barrier at the end of the k loop)
    if (KHu) pair_exchange<NT, 1>(acc, v, red + 2048, red);
    else pair_exchange<NT, 0>(acc, v, red, red + 2048);
  }
  float* zt = smem_f + TT_D_OFF / 4;                                   // fp32 z tile [group 8][224 px][8]
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int q = KHu ? S::keep_quad(1, i) : S::keep_quad(0, i);
    const int c0 = ch * 32 + q * 8 + 4 * h;
    float4 r = v[i];
    r.x = lrelu(r.x + eo[i].x); r.y = lrelu(r.y + eo[i].y); r.z = lrelu(r.z + eo[i].z); r.w = lrelu(r.w + eo[i].w);
    if (!(i < 4 ? inimg[0] : inimg[1])) r = make_float4(0.f, 0.f, 0.f, 0.f);
    st4(zt + ((c0 >> 3) * TT_NZ + (i < 4 ? zp[0] : zp[1])) * 8 + (c0 & 7), r);
    zs.v[i] = r;
  }
}

// layer 9 backward-data for a wave that carries NT (3 | 2) packed out N-tiles starting at tile T0
template <bool DBG, int NT>
__device__ __forceinline__ void turn_backward(const TurnArgs& a, unsigned char* smem, float* smem_f, int y0, int x0, int T0, int g, int ch,
                                              int kh, int lane, float smi, uint4 (&ra)[CP_RA][2]) {
  const int j = lane & 31, h = lane >> 5;
  const int Wp = a.W + 2, HWp = (a.H + 2) * Wp;
  int lo[NT], poff[NT];
  bool ok[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int e = tt_pix[(T0 + nt) * 32 + j], p = e & 255, oy = p / TT_TW, ox = p - oy * TT_TW;
    lo[nt] = (oy + 1) * TT_DP + ox + 1;
    const int y = y0 + oy, x = x0 + ox;
    ok[nt] = e < 256 && y < a.H && x < a.W;
    poff[nt] = ((y < a.H ? y : a.H - 1) + 1) * Wp + ((x < a.W ? x : a.W - 1) + 1);
  }
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
  pair_kloop<NT, TT_GRP_D, TT_PL_D, TT_DP>(acc, ra, a.wb, smem + TT_D_OFF, lo, kh, ch, lane, [](int, int) {}, [](int) {});
  {
    const float f = smi * a.winvb;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] *= f;
  }
  typedef PairSplit<NT> S;
  const int KHu = __builtin_amdgcn_readfirstlane(kh);
  const int poA = KHu ? poff[1] : poff[0], poB = poff[NT - 1];
  const bool okA = KHu ? ok[1] : ok[0], okB = ok[NT - 1];
  float4 eo[S::NQ];
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int q = KHu ? S::keep_quad(1, i) : S::keep_quad(0, i);
    const int c0 = ch * 32 + q * 8 + 4 * h;
    eo[i] = ld4(a.in + ((size_t)(c0 >> 3) * HWp + (i < 4 ? poA : poB)) * 8 + (c0 & 7));
  }
  float* red = smem_f + ((g * 2 + ch) * 2) * 1536 + lane * 4;      // input planes: dead since the forward's exchange (barriers between)
  float4 v[S::NQ];
  if (KHu) pair_exchange<NT, 1>(acc, v, red + 1536, red);
  else pair_exchange<NT, 0>(acc, v, red, red + 1536);
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int q = KHu ? S::keep_quad(1, i) : S::keep_quad(0, i);
    const int c0 = ch * 32 + q * 8 + 4 * h;
    float4 r = v[i];
    r.x *= lrelu_grad_from_out(eo[i].x); r.y *= lrelu_grad_from_out(eo[i].y);
    r.z *= lrelu_grad_from_out(eo[i].z); r.w *= lrelu_grad_from_out(eo[i].w);
    if (i < 4 ? okA : okB) st4(a.out + ((size_t)(c0 >> 3) * HWp + (i < 4 ? poA : poB)) * 8 + (c0 & 7), r);
  }
}

template <bool DBG>
__global__ void __launch_bounds__(512)
conv3x3_turn_kernel(TurnArgs a) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= a.ntiles) {             // frame role: 32 frames, 16 lanes (one DPP row) each
    const int b = ((int)blockIdx.x - a.ntiles) * TT_FRAMES + wave * 4 + (lane >> 4);
    vertex_loss_row16(b, lane & 15, a.fl);
    return;
  }
  unsigned long long t_start = 0, t_pro = 0, t_z = 0, t_st = 0, t_pl = 0;
  if (DBG) t_start = __builtin_amdgcn_s_memtime();
  LEMO_DYN_SMEM(smem_f);
  unsigned char* smem = reinterpret_cast<unsigned char*>(smem_f);
  float* wmax = reinterpret_cast<float*>(smem + TT_WMAX_OFF);        // [phase 3][wave 8] tile maxima, [3][wave] loss sums
  const int ng = wave & 1, ch = (wave >> 1) & 1, kh = wave >> 2;
  const int H = a.H, W = a.W, Wp = W + 2, HWp = (H + 2) * Wp;
  const unsigned in_gstride = (unsigned)HWp * 8u;
  int tile = (int)blockIdx.x;                    // XCD-aware tile order, as in the pair
  {
    const int q = a.ntiles >> 3, r = a.ntiles & 7, xcd = tile & 7, k = tile >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
  const int y0 = ty * TT_TH, x0 = tx * TT_TW;
  const int g = __builtin_amdgcn_readfirstlane(ng ^ kh);

  uint4 ra[CP_RA][2];
  pair_preload_a(ra, a.wf, kh, ch, lane);

  // ---- staging (the pair's plan on the 16 x 18 tile: rows y0 - 2 .., columns x0 - 3 ..; clamped onto the zero border ring)
  unsigned offB[TT_NSLOT];
  int dstB[TT_NSLOT];
#pragma unroll
  for (int k = 0; k < TT_NSLOT; ++k) {
    int c0 = tid + k * 512;
    c0 = c0 < 4 * 2 * TT_NIN ? c0 : 4 * 2 * TT_NIN - 1;
    const int gg = c0 / (2 * TT_NIN), c = c0 - gg * (2 * TT_NIN);
    const int px = c >> 1, half = c & 1;
    const int r = px / TT_INW, col = px - r * TT_INW;
    int gy = y0 - 2 + r, gx = x0 - 3 + col;
    gy = (gy < -1 ? -1 : (gy > H ? H : gy)) + 1;
    gx = (gx < -1 ? -1 : (gx > W ? W : gx)) + 1;
    const int g0 = (gg >> 1) * 4 + (gg & 1);
    offB[k] = (unsigned)g0 * in_gstride + (unsigned)(gy * Wp + gx) * 8u + 4u * half;
    dstB[k] = g0 * TT_GRP_IN + px * 16 + 8 * half;
  }
  float4 stB[TT_NSLOT];
#pragma unroll
  for (int k = 0; k < TT_NSLOT; ++k) stB[k] = ld4(a.in + offB[k]);
  float sc[2] = {1.f, 1.f}, sci[2] = {1.f, 1.f};
  {
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < TT_NSLOT; ++k) m = absmax4(stB[k], m);
    m = wave_max(m);
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    float mm = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) mm = fmaxf(mm, wmax[i]);
    f16_scale_for(mm, sc[0], sci[0]);
  }
#pragma unroll
  for (int k = 0; k < TT_NSLOT; ++k) {
    uint2 s0, s1;
    split2x4(stB[k], sc[0], s0, s1);
    *reinterpret_cast<uint2*>(smem + dstB[k]) = s0;
    *reinterpret_cast<uint2*>(smem + dstB[k] + TT_PL_IN) = s1;
  }
#pragma unroll
  for (int k = 0; k < TT_NSLOT; ++k) stB[k] = ld4(a.in + 2u * in_gstride + offB[k]);
  __syncthreads();
  if (DBG) t_pro = __builtin_amdgcn_s_memtime();

  // ---- layer 9 forward: z on 14 x 16 -------------------------------------------------------------------------------------------
  TurnZ zs;
  if (g) turn_forward<3>(a, smem, smem_f, wmax, y0, x0, 1, ch, kh, lane, wave, ra, sc, sci, stB, dstB, zs);
  else turn_forward<4>(a, smem, smem_f, wmax, y0, x0, 0, ch, kh, lane, wave, ra, sc, sci, stB, dstB, zs);
  pair_preload_a(ra, a.wb, kh, ch, lane);                  // the backward's first weight fragments travel during the stencil
  __syncthreads();                                         // z tile complete
  if (DBG) t_z = __builtin_amdgcn_s_memtime();

  // ---- stencil: d(pre-act 10) on 14 x 14 (smooth_loss_body's arithmetic), loss partial over the owned pixels ---------------------
  const float* zt = smem_f + TT_D_OFF / 4;
  float4 dv[TT_KITEM];
  int dslot[TT_KITEM];
  float sq = 0.f, mloc = 0.f;
#pragma unroll
  for (int k = 0; k < TT_KITEM; ++k) {
    const int it = tid + k * 512, ic = it < TT_NITEM ? it : TT_NITEM - 1;
    const int half = ic & 1, rest = ic >> 1, gq = rest / TT_ND, dp = rest - gq * TT_ND;
    const int dr = dp / TT_DW, dc = dp - dr * TT_DW;
    const int y = y0 - 1 + dr, x = x0 - 1 + dc;
    const bool valid = it < TT_NITEM && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    const bool own = valid && dr >= 1 && dr <= TT_TH && dc >= 1 && dc <= TT_TW;
    const bool hasl = x >= 1, hasr = x <= W - 2;
    const float* zc = zt + (gq * TT_NZ + dr * TT_ZW + dc + 1) * 8 + 4 * half;
    const float4 c = ld4(zc), l = ld4(zc - 8), r = ld4(zc + 8);
    float4 gr = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hasl) { gr.x += c.x - l.x; gr.y += c.y - l.y; gr.z += c.z - l.z; gr.w += c.w - l.w; }
    if (hasr) {
      const float d0 = r.x - c.x, d1 = r.y - c.y, d2 = r.z - c.z, d3 = r.w - c.w;
      if (own) sq += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      gr.x -= d0; gr.y -= d1; gr.z -= d2; gr.w -= d3;
    }
    const float cf = a.coef2;
    float4 o = make_float4(cf * gr.x * lrelu_grad_from_out(c.x), cf * gr.y * lrelu_grad_from_out(c.y),
                           cf * gr.z * lrelu_grad_from_out(c.z), cf * gr.w * lrelu_grad_from_out(c.w));
    if (!valid) o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.dpre && own) st4(a.dpre + ((size_t)gq * HWp + (y + 1) * Wp + (x + 1)) * 8 + 4 * half, o);
    dv[k] = o;
    dslot[k] = it < TT_NITEM ? gq * TT_GRP_D + (dr * TT_DP + dc) * 16 + 8 * half : -1;
    mloc = absmax4(o, mloc);
  }
  mloc = wave_max(mloc);
  sq = wave_sum(sq);
  if (lane == 0) { wmax[16 + wave] = mloc; wmax[24 + wave] = sq; }
  __syncthreads();                                         // every z read is done: the dpre planes may overwrite the z tile
  if (DBG) t_st = __builtin_amdgcn_s_memtime();
  float sm, smi;
  {
    float mm = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) mm = fmaxf(mm, wmax[16 + i]);
    f16_scale_for(mm, sm, smi);
  }
  if (tid == 0 && a.acc) {
    const float s = ((((((wmax[24] + wmax[25]) + wmax[26]) + wmax[27]) + wmax[28]) + wmax[29]) + wmax[30]) + wmax[31];
    atomicAdd(a.acc + (blockIdx.x & 31) * 16, (double)s);
  }
#pragma unroll
  for (int k = 0; k < TT_KITEM; ++k) {
    if (dslot[k] < 0) continue;
    uint2 s0, s1;
    split2x4(dv[k], sm, s0, s1);
    *reinterpret_cast<uint2*>(smem + TT_D_OFF + dslot[k]) = s0;
    *reinterpret_cast<uint2*>(smem + TT_D_OFF + dslot[k] + TT_PL_D) = s1;
  }
  __syncthreads();
  if (DBG) t_pl = __builtin_amdgcn_s_memtime();

  // ---- layer 9 backward-data on the 144 owned pixels ------------------------------------------------------------------------------
  if (g) turn_backward<DBG, 2>(a, smem, smem_f, y0, x0, 3, 1, ch, kh, lane, smi, ra);
  else turn_backward<DBG, 3>(a, smem, smem_f, y0, x0, 0, 0, ch, kh, lane, smi, ra);
  {                                                        // act[10]: the owned z (deferred: a store before the barriers is waited for)
    const int KHu = __builtin_amdgcn_readfirstlane(kh), h = lane >> 5;
    const int nq = g ? PairSplit<3>::NQ : PairSplit<4>::NQ;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i >= nq) continue;
      const int q = g ? (KHu ? PairSplit<3>::keep_quad(1, i) : PairSplit<3>::keep_quad(0, i))
                      : (KHu ? PairSplit<4>::keep_quad(1, i) : PairSplit<4>::keep_quad(0, i));
      const int c0 = ch * 32 + q * 8 + 4 * h;
      if (i < 4 ? zs.own[0] : zs.own[1]) st4(a.z + ((size_t)(c0 >> 3) * HWp + (i < 4 ? zs.po[0] : zs.po[1])) * 8 + (c0 & 7), zs.v[i]);
    }
  }
  if (DBG && lane == 0) {
    unsigned long long* r = a.dbg + ((size_t)blockIdx.x * 8 + wave) * 8;
    r[0] = __builtin_amdgcn_s_getreg(63492);
    r[1] = t_start; r[2] = t_pro; r[3] = t_z; r[4] = t_st; r[5] = t_pl; r[6] = __builtin_amdgcn_s_memtime(); r[7] = 0;
  }
}

int conv_turn_init() {
  static LdsOptinOnce once;
  return lds_optin(once, {{&conv3x3_turn_kernel<false>, TT_SMEM}, {&conv3x3_turn_kernel<true>, TT_SMEM}});
}

bool conv3x3_turn_supported(int H, int W) { return H >= 1 && W >= 2 && (long)H * W <= (1l << 24); }

int conv3x3_turn_tiles(int H, int W) { return ((W + TT_TW - 1) / TT_TW) * ((H + TT_TH - 1) / TT_TH); }

// act[9] -> [layer 9 forward] -> z (owned interior -> act[10]) -> d(pre-act 10) = coef2 * stencil * lrelu'(z) -> [layer 9 backward-data]
// -> d(pre-act 9) = conv^T * lrelu'(act[9]).  acc: f64 [32 slots][16], the sum of squares lands in slot element 0 (may be null: no loss);
// dpre (may be null): d(pre-act 10) of every image pixel; fl (may be null): the per-frame losses as extra workgroups.
int conv3x3_turn_f16(const float* in, const void* wf, float winvf, const float* bias, const void* wb, float winvb, float* z, float* out,
                     double* acc, float coef2, int H, int W, float* dpre, const FrameLoss* fl, hipStream_t s, unsigned long long* dbg) {
  if (!conv3x3_turn_supported(H, W)) return LEMO_ERR_SHAPE;
  if (!in || !wf || !wb || !bias || !z || !out || !(winvf > 0.f) || !(winvb > 0.f)) return LEMO_ERR_ARG;
  if (fl && (fl->B < 1 || dbg)) return LEMO_ERR_ARG;
  if (int rc = conv_turn_init()) return rc;
  TurnArgs a{};
  a.in = in; a.wf = reinterpret_cast<const uint4*>(wf); a.wb = reinterpret_cast<const uint4*>(wb); a.bias = bias;
  a.z = z; a.out = out; a.dpre = dpre; a.acc = acc; a.winvf = winvf; a.winvb = winvb; a.coef2 = coef2; a.H = H; a.W = W;
  a.ntx = (W + TT_TW - 1) / TT_TW;
  a.ntiles = conv3x3_turn_tiles(H, W);
  if (fl) { a.fl = *fl; a.nfb = (fl->B + TT_FRAMES - 1) / TT_FRAMES; }
  a.dbg = dbg;
  if (dbg) hipLaunchKernelGGL((conv3x3_turn_kernel<true>), dim3(a.ntiles), dim3(512), TT_SMEM, s, a);
  else hipLaunchKernelGGL((conv3x3_turn_kernel<false>), dim3(a.ntiles + a.nfb), dim3(512), TT_SMEM, s, a);
  return (int)hipGetLastError();
}

}  // namespace lemo
