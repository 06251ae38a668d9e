// Device machinery of the fused two-layer kernels (conv_pair_kernels.hip, conv_turn_kernels.hip): the K-half split / exchange of
// the accumulators, the bank-conflict-free lane -> column map of an N-tile, and the K loop over one K half (weights from L2 through
// a ring, activation fragments from split-f16 LDS planes).  Shared as header code so both kernels compile the same loop.
#pragma once
#include "conv_f16.hpp"

namespace lemo {

// which (tile, quad) pairs of its partial sums K-half KH finishes itself ("keep") and which it hands to the other half ("give"):
// NT tiles x 4 quads (a quad = 4 consecutive couts of one column = accumulator registers 4 q .. 4 q + 3).
// NT 3: KH keeps tile KH and half of tile 2 (quads 2 KH, 2 KH + 1); NT 2: KH keeps tile KH; NT 4 (conv_turn_kernels.hip): tiles KH, 2 + KH.
template <int NT> struct PairSplit {
  static constexpr int NQ = NT == 4 ? 8 : (NT == 3 ? 6 : 4);
  static constexpr int keep_tile(int KH, int i) { return i < 4 ? KH : (NT == 4 ? 2 + KH : 2); }
  static constexpr int keep_quad(int KH, int i) { return i < 4 ? i : (NT == 4 ? i - 4 : (i - 4) + 2 * KH); }
  static constexpr int give_tile(int KH, int i) { return i < 4 ? 1 - KH : (NT == 4 ? 3 - KH : 2); }
  static constexpr int give_quad(int KH, int i) { return i < 4 ? i : (NT == 4 ? i - 4 : (i - 4) + 2 * (1 - KH)); }
};

// hand the "give" quads to the partner wave through LDS, add the partner's to the "keep" quads in the fixed order kh 0 + kh 1
// (The __syncthreads() below is reached through differently specialised inlined copies of this function -- NT 3 | 2, KH 0 | 1 -- i.e. the
// waves of a workgroup meet at different s_barrier instructions.  gfx9's s_barrier counts waves, not call sites, and the host emulator
// does the same; ADVICE r04 asked for ONE call site at kernel scope.  Round 5 built that (exchange split into give / keep around a
// barrier in the kernel body, layer 2 split into two halves) and measured it: bit-identical results, but +1.0 us per pair on the same
// box, interleaved (fwd 25.6 vs 24.5, bwd 23.7 vs 22.8 us) and SQ_LDS_BANK_CONFLICT 5.2e5 -> 1.09e6 per launch (profiles/r05_pmc_summary.txt
// of commit 1121d81 vs r04) -- the merged control flow costs the layer-2 epilogue its schedule.  Reverted; the form below stays.)
template <int NT, int KH, int NA, int NV>
__device__ __forceinline__ void pair_exchange(const f32x16 (&acc)[NA], float4 (&v)[NV], float* red_mine, const float* red_theirs) {
  typedef PairSplit<NT> S;
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int t = S::give_tile(KH, i), q = S::give_quad(KH, i);
    st4(red_mine + i * 256, make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]));
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < S::NQ; ++i) {
    const int t = S::keep_tile(KH, i), q = S::keep_quad(KH, i);
    const float4 o = ld4(red_theirs + i * 256);
    const float4 m = make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
    v[i] = KH ? make_float4(o.x + m.x, o.y + m.y, o.z + m.z, o.w + m.w) : make_float4(m.x + o.x, m.y + o.y, m.z + o.z, m.w + o.w);
  }
}

// An MFMA N-tile = 2 rows x 16 columns of a grid with row pitch 18 (layer 1: the 12 x 16 mid grid read from the 14 x 18 input
// planes; layer 2: the 10 x 16 "virtual" out grid -- columns -1 .. 14 of the out tile, two of them padding -- read from the mid planes,
// stored with the same pitch).  ds_read_b128 serves a wave in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32), and a
// group is conflict-free iff its 16 lanes hit 16 distinct 16-byte slots mod 16 (MI355X_MICROARCH.md, LDS).  With lane j <-> column j
// in both rows the second row sits 18 = 16 + 2 slots further and two slots of every group collide (measured: SQ_LDS_BANK_CONFLICT =
// 47 % of SQ_LDS_IDX_ACTIVE).  Rotating the second row's columns by 2 -- lane 16 + i <-> column (i - 2) mod 16 -- makes lane j's
// slot == j + const (mod 16) for all 32 lanes: conflict-free for every tap.
__device__ __forceinline__ int cp_lane_col(int j) { return j < 16 ? j : ((j - 18) & 15); }

#define CP_RA 3          // weight-fragment ring: requested CP_RA - 1 steps ahead (conv_split_kernels.hip: deeper measured slower)

// K loop of one layer over one K half (2 k-chunks x 9 taps = 18 steps) for NT N-tiles: A = weights from L2 through the ring,
// B = activation fragments from LDS planes at `bbase` (group stride GRP, piece stride PL, row pitch PITCH), one step ahead.
// STAGE (layer 1 only): the second staging phase rides inside the first k-chunk (see the kernel body).
// the first CP_RA - 1 weight fragments of a K loop: requested by the caller as early as it knows the layer (they come from L2,
// ~700 cycles away: layer 2's are requested before the K-half exchange of layer 1, not at the top of its own loop)
__device__ __forceinline__ void pair_preload_a(uint4 (&ra)[CP_RA][2], const uint4* __restrict__ w, int kh, int ch, int lane) {
#pragma unroll
  for (int u0 = 0; u0 < CP_RA - 1; ++u0)
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) ra[u0][s_] = w[(unsigned)((((2 * kh) * 9 + u0) * 2 + ch) * 2 + s_) * 64u + lane];
}

template <int NT, int GRP, int PL, int PITCH, int NA, typename MidFn, typename EndFn>
__device__ __forceinline__ void pair_kloop(f32x16 (&acc)[NA], uint4 (&ra)[CP_RA][2], const uint4* __restrict__ w, const unsigned char* bbase,
                                           const int (&li)[NA], int kh, int ch, int lane, MidFn&& mid_fn, EndFn&& end_fn) {
  const int h = lane >> 5;
  uint4 rb[2][NT][2];
#define CP_LOAD_A(SET, U)                                                                              \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                                     \
    ra[SET][s_] = w[(unsigned)((((2 * kh + (U) / 9) * 9 + (U) % 9) * 2 + ch) * 2 + s_) * 64u + lane];
#define CP_LOAD_B(SET, U)                                                                              \
  _Pragma("unroll") for (int nt_ = 0; nt_ < NT; ++nt_)                                                 \
    _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                                   \
      rb[SET][nt_][s_] = *reinterpret_cast<const uint4*>(                                              \
          bbase + (2 * (2 * kh + (U) / 9) + h) * GRP + s_ * PL + (li[nt_] + (((U) % 9) / 3 - 1) * PITCH + (((U) % 9) % 3 - 1)) * 16);
#define CP_MFMA1(SA, SETA, SB, SETB)                                                                   \
  _Pragma("unroll") for (int nt_ = 0; nt_ < NT; ++nt_)                                                 \
    acc[nt_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ra[SETA][SA]),         \
                                                      __builtin_bit_cast(f16x8, rb[SETB][nt_][SB]), acc[nt_], 0, 0, 0);
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    CP_LOAD_B((cc * 9) & 1, cc * 9)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int u = cc * 9 + tap;
      if (u + CP_RA - 1 < 18) { CP_LOAD_A((u + CP_RA - 1) % CP_RA, u + CP_RA - 1) }
      if (tap + 1 < 9) { CP_LOAD_B((u + 1) & 1, u + 1) }
      __builtin_amdgcn_sched_barrier(0);
      CP_MFMA1(0, u % CP_RA, 1, u & 1) CP_MFMA1(1, u % CP_RA, 0, u & 1) CP_MFMA1(0, u % CP_RA, 0, u & 1)   // smallest products first
      mid_fn(cc, tap);
      __builtin_amdgcn_sched_barrier(0);
    }
    end_fn(cc);
  }
#undef CP_LOAD_A
#undef CP_LOAD_B
#undef CP_MFMA1
}

}  // namespace lemo
