// VPoser encoder (human_body_prior/train/vposer_smpl.py:98-105) in eval mode, forward and input gradient, one launch each:
//     x [B][63] -> bn1 -> fc1 63->512 -> lrelu(0.2) -> bn2 -> fc2 512->512 -> lrelu(0.2) -> mean = mu(h2), std = softplus(logvar(h2))
// Dropout is the identity and BatchNorm uses its running statistics, so bn1 is folded into fc1 and bn2 into fc2 (weights and bias)
// at pack time, in float64, rounded once (lemo_amd.vposer.pack_vposer_enc).  The two heads are ONE 512 -> 64 layer (mu rows 0..31,
// logvar rows 32..63).  The backward is the mirror image on the transposed packs: 64 -> 512 -> 512 -> 64 (63 written).
//
// Arithmetic: v_mfma_f32_16x16x4_f32, the exact fp32 MFMA (a k-ordered fmaf chain: deterministic, one fixed reduction order per output).
// As in gemm_kernels.hip the weights are the A operand (rows = output neurons) and the activations the B operand (columns = batch
// rows), so a lane ends with four consecutive neurons of one batch row: one 16-byte store into LDS and into h1 / h2.
//
// Tile: a workgroup (4 waves) owns 32 batch rows; wave w owns neurons 128 w .. 128 w + 127 of a hidden layer for ALL 32 rows (8 m-tiles
// x 2 n-tiles = 16 accumulators, 64 registers) and head neurons 16 w .. 16 w + 15.  A whole layer's output is held in accumulators, so
// ONE [32][516] LDS buffer (66 KB) serves x, h1 and h2 in turn (barrier, overwrite, barrier) and no hidden activation is read back from
// global memory.  Why 32 rows:
//  * an A fragment (a weight) is used for rows / 16 MFMAs.  A wave needs 8 x 1 KB of weights per 16-deep k chunk; at 32 rows that is
//    64 MFMAs = 2048 cycles of matrix pipe, i.e. 16 B/clk per CU at full rate: half of what a CU takes in from L2 (MI355X_MICROARCH
//    "Indexed rows": 66-73 GB/s per CU, ~29 B/clk).  16 rows would need 32 B/clk (the launch would wait for weights), 64 rows need
//    8 B/clk but 132 KB of LDS and 128 accumulator registers: one workgroup per CU and half as many workgroups for a small batch;
//  * 66 KB lets two workgroups share a CU (2 waves per SIMD, < 256 registers each), so one workgroup's barriers and epilogues sit
//    beside the other's MFMAs; 16 independent accumulators per wave cover the 40-cycle dependent latency of the 16x16x4 form;
//  * B = 119 (a fitting window) is 4 workgroups of 32 x 2560 matrix-pipe cycles ~ 34 us at the issue rate (not measured here: see
//    DESIGN.md for the measured figures); the target is throughput at tens of thousands of rows.
// The waves of a workgroup split the NEURONS, so no weight is needed by two waves and there is nothing to share through LDS: the
// weights are instead packed on the host in fragment order, P[k chunk][m-tile][lane][4] (lane = 16 q + i holds W[16 mt + i][16 c + 4 q ..
// + 3]), which makes every A-fragment load one fully coalesced 1 KB dwordx4 wave-load out of L2 (the 1.3 MB of packs stay resident in
// every XCD's 4 MB L2).  The fragments of chunk c + 1 are requested before the MFMAs of chunk c.
//
// K = 63 is padded to 64 inside the kernel: column 63 of the x tile is written as 0 and never read from memory (the packed fc1 has a
// zero column there too).  Rows of a ragged last tile are zero in LDS and are never loaded or stored.  Rows are mapped onto
// blockIdx.x only (no 65 535 limit) and every row offset is formed in 64 bits.
#include "kernels.hpp"

namespace lemo {

constexpr int ENC_ROWS = 32, ENC_LD = 516;          // LDS row stride 516 floats: 129 16-byte slots, rows i and i + 1 one slot apart

// acc[mt][nt] += W[(wave MT + mt) 16 .. + 15][:] . act[nt 16 .. + 15][:] over NCH chunks of 16 k; Wp in fragment order, 4 MT m-tiles per chunk
template <int MT, int NCH>
__device__ __forceinline__ void enc_gemm(const float* __restrict__ Wp, const float* act, int wave, int lane, f32x4 (&acc)[MT][2]) {
  const int i = lane & 15, q = lane >> 4;
  const float* wp = Wp + ((size_t)(wave * MT) * 64 + lane) * 4;
  const float* bp = act + i * ENC_LD + 4 * q;
  constexpr int CSTEP = 4 * MT * 256;                // floats per chunk: 4 MT m-tiles x 64 lanes x 4
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 a[MT], an[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) a[mt] = ld4(wp + mt * 256);
#pragma unroll 1
  for (int c = 0; c < NCH; ++c) {
    const int cn = (c + 1 < NCH) ? c + 1 : c;        // clamp: unconditional loads
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) an[mt] = ld4(wp + (size_t)cn * CSTEP + mt * 256);
    float4 b[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) b[nt] = ld4(bp + nt * 16 * ENC_LD + c * 16);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt].x, b[nt].x, acc[mt][nt], 0, 0, 0);
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt].y, b[nt].y, acc[mt][nt], 0, 0, 0);
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt].z, b[nt].z, acc[mt][nt], 0, 0, 0);
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt].w, b[nt].w, acc[mt][nt], 0, 0, 0);
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
  }
}

// a hidden layer's epilogue: every value through f(tile row n, first neuron m0, the four values) and into the LDS tile.
// D: col = n (lane & 15), rows 4 q + r -> neuron
template <typename F>
__device__ __forceinline__ void enc_hidden_epilogue(const f32x4 (&acc)[8][2], float* act, int wave, int lane, F f) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int n = nt * 16 + i, m0 = (wave * 8 + mt) * 16 + 4 * q;
      st4(act + n * ENC_LD + m0, f(n, m0, make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3])));
    }
}

// torch.nn.functional.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus20(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus20_grad(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }

__global__ void __launch_bounds__(256)
vposer_enc_fwd_kernel(VPoserEncW w, const float* __restrict__ pin, int pin_stride, int B, float* __restrict__ mean, float* __restrict__ stdv,
                      int out_stride, float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ lv) {
  __shared__ __attribute__((aligned(16))) float act[ENC_ROWS * ENC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * ENC_ROWS;
  {                                                  // x tile: 8 floats per thread, zero in column 63 and in rows >= B
    const int r = tid >> 3, c0 = (tid & 7) * 8;
    const long long row = row0 + r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      act[r * ENC_LD + c] = (row < B && c < 63) ? pin[(size_t)row * pin_stride + c] : 0.f;
    }
  }
  __syncthreads();
  f32x4 acc[8][2];
  enc_gemm<8, 4>(w.w1p, act, wave, lane, acc);
  __syncthreads();                                   // every wave has read x
  enc_hidden_epilogue(acc, act, wave, lane, [&](int n, int m0, float4 v) {
    const float4 bb = ld4(w.b1 + m0);
    v.x = lrelu(v.x + bb.x); v.y = lrelu(v.y + bb.y); v.z = lrelu(v.z + bb.z); v.w = lrelu(v.w + bb.w);
    if (h1 && row0 + n < B) st4(h1 + (size_t)(row0 + n) * 512 + m0, v);
    return v;
  });
  __syncthreads();
  enc_gemm<8, 32>(w.w2p, act, wave, lane, acc);
  __syncthreads();                                   // every wave has read h1
  enc_hidden_epilogue(acc, act, wave, lane, [&](int n, int m0, float4 v) {
    const float4 bb = ld4(w.b2 + m0);
    v.x = lrelu(v.x + bb.x); v.y = lrelu(v.y + bb.y); v.z = lrelu(v.z + bb.z); v.w = lrelu(v.w + bb.w);
    if (h2 && row0 + n < B) st4(h2 + (size_t)(row0 + n) * 512 + m0, v);
    return v;
  });
  __syncthreads();
  f32x4 ah[1][2];
  enc_gemm<1, 32>(w.whp, act, wave, lane, ah);       // head neuron 16 wave + 4 q + r: waves 0, 1 = mu, waves 2, 3 = logvar
  const int i = lane & 15, q = lane >> 4, m0 = wave * 16 + 4 * q, j0 = m0 & 31;
  const float4 bb = ld4(w.bh + m0);
  const float bias[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const long long row = row0 + nt * 16 + i;
    if (row < B) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = ah[0][nt][r] + bias[r];
        if (wave < 2) mean[(size_t)row * out_stride + j0 + r] = v;
        else {
          if (lv) lv[(size_t)row * 32 + j0 + r] = v;
          stdv[(size_t)row * out_stride + j0 + r] = softplus20(v);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256)
vposer_enc_bwd_kernel(VPoserEncW w, const float* __restrict__ h1, const float* __restrict__ h2, const float* __restrict__ lv,
                      const float* __restrict__ d_mean, const float* __restrict__ d_std, int out_stride, int B, float* __restrict__ dpin,
                      int pin_stride) {
  __shared__ __attribute__((aligned(16))) float act[ENC_ROWS * ENC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * ENC_ROWS;
  {                                                  // d(head) tile [32][64]: d_mean | d_std * softplus'(lv); a null gradient is zero
    const int r = tid >> 3, c0 = (tid & 7) * 8;
    const long long row = row0 + r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e, j = c & 31;
      float v = 0.f;
      if (row < B) {
        if (c < 32) { if (d_mean) v = d_mean[(size_t)row * out_stride + j]; }
        else if (d_std) v = d_std[(size_t)row * out_stride + j] * softplus20_grad(lv[(size_t)row * 32 + j]);
      }
      act[r * ENC_LD + c] = v;
    }
  }
  __syncthreads();
  f32x4 acc[8][2];
  enc_gemm<8, 4>(w.whtp, act, wave, lane, acc);      // d(h2) = head^T d(head)
  __syncthreads();
  auto through_lrelu = [&](const float* h) {
    return [=](int n, int m0, float4 v) {
      if (row0 + n < B) {                            // rows past B are zero already
        const float4 y = ld4(h + (size_t)(row0 + n) * 512 + m0);
        v.x *= lrelu_grad_from_out(y.x); v.y *= lrelu_grad_from_out(y.y); v.z *= lrelu_grad_from_out(y.z); v.w *= lrelu_grad_from_out(y.w);
      }
      return v;
    };
  };
  enc_hidden_epilogue(acc, act, wave, lane, through_lrelu(h2));
  __syncthreads();
  enc_gemm<8, 32>(w.w2tp, act, wave, lane, acc);     // d(h1) = fc2'^T d(pre-activation 2)
  __syncthreads();
  enc_hidden_epilogue(acc, act, wave, lane, through_lrelu(h1));
  __syncthreads();
  f32x4 ax[1][2];
  enc_gemm<1, 32>(w.w1tp, act, wave, lane, ax);      // d(x) = fc1'^T d(pre-activation 1): input column 16 wave + 4 q + r
  const int i = lane & 15, q = lane >> 4, c0 = wave * 16 + 4 * q;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const long long row = row0 + nt * 16 + i;
    if (row < B) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (c0 + r < 63) dpin[(size_t)row * pin_stride + c0 + r] = ax[0][nt][r];
    }
  }
}

int vposer_encode_fwd(const VPoserEncW& w, const float* pin, int pin_stride, int B, float* mean, float* stdv, int out_stride,
                      float* h1, float* h2, float* lv, hipStream_t s) {
  if (B <= 0 || !pin || !mean || !stdv || pin_stride < 63 || out_stride < 32 || !w.w1p || !w.b1 || !w.w2p || !w.b2 || !w.whp || !w.bh)
    return LEMO_ERR_ARG;
  const unsigned grid = (unsigned)(((long long)B + ENC_ROWS - 1) / ENC_ROWS);
  hipLaunchKernelGGL(vposer_enc_fwd_kernel, dim3(grid), dim3(256), 0, s, w, pin, pin_stride, B, mean, stdv, out_stride, h1, h2, lv);
  return (int)hipGetLastError();
}

int vposer_encode_bwd(const VPoserEncW& w, const float* h1, const float* h2, const float* lv, const float* d_mean, const float* d_std,
                      int out_stride, int B, float* dpin, int pin_stride, hipStream_t s) {
  if (B <= 0 || !h1 || !h2 || !lv || !dpin || pin_stride < 63 || out_stride < 32 || !w.w1tp || !w.w2tp || !w.whtp) return LEMO_ERR_ARG;
  const unsigned grid = (unsigned)(((long long)B + ENC_ROWS - 1) / ENC_ROWS);
  hipLaunchKernelGGL(vposer_enc_bwd_kernel, dim3(grid), dim3(256), 0, s, w, h1, h2, lv, d_mean, d_std, out_stride, B, dpin, pin_stride);
  return (int)hipGetLastError();
}

}  // namespace lemo
