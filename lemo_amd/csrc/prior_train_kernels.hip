// Kernels of the smoothness-prior training step (models/AE_sep.py Enc + Dec, train_smooth_prior.py:96-136) that the
// inference path does not have: the batched 3x3 weight gradient, the decoder's 1-channel end fused with the L1 term, the
// batched loss reductions, Adam over the flat parameter vector and the on-device repack of the conv weight packs.
// Forward and backward-data of the 32/64-channel layers stay on conv3x3_mfma_lds (conv_kernels.hip).
//
// Weight gradient as a GEMM (one form for both modules).  With A, B CG8P activations of one batch,
//   out[m][n][t] = sum_{b, y, x} A_b[m][y][x] * B_b[n][y + ky - 1][x + kx - 1],   t = 3 ky + kx,
// M = channels of A (32 / 64), N = 9 x channels of B (288 / 576), K = bs * H * W (2.0 M at bs = 60, 245 x 135).
//   Enc conv l  (weight [cout][cin][3][3]):  A = d(pre-activation of its output), B = its input;  bias grad = sum A.
//   Dec deconv j (weight [nin][nout][3][3], stride 1, padding 1): dW[i][o][ky][kx] = sum in[i][p] dout[o][p + (ky-1, kx-1)], so
//               A = its input, B = d(pre-activation of its output);  bias grad = sum B.
// In both cases `out` is the parameter's own [M][N][3][3] layout, so the reduction writes straight into the gradient vector.
#include "kernels.hpp"

namespace lemo {

// ---------------------------------------------------------------------------------------------------------------------
// batched weight gradient on v_mfma_f32_32x32x2_f32
// ---------------------------------------------------------------------------------------------------------------------
// Work split: the bs * H image rows are dealt to nwg workgroups in contiguous runs (fixed, independent of timing).  Per row a
// workgroup stages A's row (MA channels x (W + 2) padded positions, zero border columns included) and B's three padded rows
// around it (NB channels x 3 (W + 2)) channel-major in LDS; K runs over the padded positions of the row (the border columns
// of A are zero, so they add nothing), tap t reads B at position k + ky (W + 2) + kx of the staged rows.  Each of the 4 waves
// owns one 32 x 32 (m, n) tile for all 9 taps (9 accumulators = 144 AGPRs) and, when the layer has fewer than 4 tiles, every
// (4 / tiles)-th K step.  Each wave stores its tiles as a partial; sp_wgrad_reduce_kernel sums partials in workgroup order,
// then K-slice order: no float atomics, bit-identical runs.
#define SPW_PSZ (4 * 9 * 1024 + 64)          // floats of one workgroup's partial: [wave][tap][32][32] + bias[64]

__host__ __device__ static inline int spw_kp(int W) { return (W + 3) & ~1; }                  // K steps of 2 positions cover W + 2
__host__ __device__ static inline int spw_la(int W) { return spw_kp(W) + 1; }                  // odd LDS row strides
__host__ __device__ static inline int spw_lb(int W) { const int l = 3 * (W + 2) + 3; return l | 1; }
static inline int spw_smem_bytes(int W, int ma, int nb) { return (ma * spw_la(W) + nb * spw_lb(W)) * 4; }
#define SPW_MAX_SMEM (160 * 1024)

struct SpWgradArgs { const float* A; const float* B; size_t a_stride, b_stride; float* part; int bs, H, W, bias_b, nwg; };

template <int MA, int NB>
__global__ void __launch_bounds__(256)
sp_wgrad_mfma_kernel(SpWgradArgs q) {
  LEMO_DYN_SMEM(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = q.W, Wp = W + 2, HWp = (q.H + 2) * Wp;
  const int KP = spw_kp(W), LA = spw_la(W), LB = spw_lb(W);
  float* As = smem;                               // [MA][LA]: A at padded positions 0 .. Wp-1 of the row, zero beyond
  float* Bs = smem + MA * LA;                     // [NB][LB]: 0, B at the 3 Wp positions of padded rows y .. y+2, zeros
  for (int i = tid; i < MA * LA; i += 256) As[i] = 0.f;
  for (int i = tid; i < NB * LB; i += 256) Bs[i] = 0.f;

  constexpr int NTM = MA / 32, NTN = NB / 32, NT = NTM * NTN, KW = 4 / NT;
  const int tile = wave % NT, kw = wave / NT;
  const int mt = tile / NTN, nt = tile % NTN;
  const float* ap = As + (mt * 32 + (lane & 31)) * LA + (lane >> 5);
  const float* bp = Bs + (nt * 32 + (lane & 31)) * LB + (lane >> 5);
  int toff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) toff[t] = (t / 3) * Wp + (t % 3);

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bacc = 0.f;                               // bias: channel tid & 63, positions = (tid >> 6) mod 4
  const int bch = tid & 63, bpart = tid >> 6, nbias = q.bias_b ? NB : MA;

  const int total = q.bs * q.H;
  const int r0 = (int)((long long)blockIdx.x * total / q.nwg), r1 = (int)((long long)(blockIdx.x + 1) * total / q.nwg);
  for (int row = r0; row < r1; ++row) {
    const int b = row / q.H, y = row - b * q.H;
    const float* A = q.A + (size_t)b * q.a_stride;
    const float* B = q.B + (size_t)b * q.b_stride;
    __syncthreads();                              // the previous row's MFMAs are done with the staged operands
    for (int i = tid; i < (MA / 8) * Wp * 2; i += 256) {
      const int g = i / (2 * Wp), rem = i - g * 2 * Wp, xp = rem >> 1, h = rem & 1;
      const float4 v = ld4(A + ((size_t)g * HWp + (size_t)(y + 1) * Wp + xp) * 8 + 4 * h);
      float* d = As + (g * 8 + 4 * h) * LA + xp;
      d[0] = v.x; d[LA] = v.y; d[2 * LA] = v.z; d[3 * LA] = v.w;
    }
    for (int i = tid; i < (NB / 8) * 3 * Wp * 2; i += 256) {
      const int g = i / (6 * Wp), rem = i - g * 6 * Wp, j = rem >> 1, h = rem & 1;
      const float4 v = ld4(B + ((size_t)g * HWp + (size_t)y * Wp + j) * 8 + 4 * h);
      float* d = Bs + (g * 8 + 4 * h) * LB + 1 + j;
      d[0] = v.x; d[LB] = v.y; d[2 * LB] = v.z; d[3 * LB] = v.w;
    }
    __syncthreads();
    if (bch < nbias) {
      const float* src = q.bias_b ? Bs + bch * LB + 1 + Wp : As + bch * LA;     // B: the centre row is this image row
      for (int xp = bpart; xp < Wp; xp += 4) bacc += src[xp];
    }
    for (int s = kw; s < KP / 2; s += KW) {
      const float a = ap[2 * s];
      float bv[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) bv[t] = bp[2 * s + toff[t]];
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[t], acc[t], 0, 0, 0);
    }
  }

  float* part = q.part + (size_t)blockIdx.x * SPW_PSZ;
  float* pw = part + wave * 9 * 1024;
  const int j = lane & 31, ih = 4 * (lane >> 5);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) pw[t * 1024 + ((r & 3) + 8 * (r >> 2) + ih) * 32 + j] = acc[t][r];
  __syncthreads();
  smem[tid] = bacc;
  __syncthreads();
  if (tid < nbias) part[4 * 9 * 1024 + tid] = ((smem[tid] + smem[64 + tid]) + smem[128 + tid]) + smem[192 + tid];
}

// gw[(m NB + n) 9 + t] = sum over workgroups, then K slices, of the wave partials; gb[c] = sum over workgroups
template <int MA, int NB>
__global__ void __launch_bounds__(256)
sp_wgrad_reduce_kernel(const float* __restrict__ part, int nwg, int bias_b, float* __restrict__ gw, float* __restrict__ gb) {
  constexpr int NTN = NB / 32, NT = (MA / 32) * NTN, KW = 4 / NT;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int nw = 9 * MA * NB, nbias = bias_b ? NB : MA;
  if (e < nw) {
    const int t = e / (MA * NB), mn = e - t * MA * NB, m = mn / NB, n = mn - m * NB;      // n fastest: coalesced partial reads
    const int tile = (m >> 5) * NTN + (n >> 5);
    const size_t o = (size_t)t * 1024 + (m & 31) * 32 + (n & 31);
    float s = 0.f;
    for (int w = 0; w < nwg; ++w)
#pragma unroll
      for (int k = 0; k < KW; ++k) s += part[(size_t)w * SPW_PSZ + (size_t)(tile + NT * k) * 9216 + o];
    gw[(size_t)mn * 9 + t] = s;
  } else if (e < nw + nbias) {
    const int c = e - nw;
    float s = 0.f;
    for (int w = 0; w < nwg; ++w) s += part[(size_t)w * SPW_PSZ + 4 * 9 * 1024 + c];
    gb[c] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1-channel layers (Enc layer 0, Dec 32 -> 1 and 1 -> 1): plain FMAs, same contraction with NB = 1
// ---------------------------------------------------------------------------------------------------------------------
// A: CA = 32 channels in CG8P or CA = 1 plain padded image [(H+2)(W+2)]; B: plain padded image.  Block (blk, b) covers a
// contiguous pixel range of image b; thread = (channel tid % CA, pixel lane tid / CA).  Partial per block: [CA][9 taps,
// sum A] + sum B, reduced in block order by sp_wgrad_c1_reduce_kernel.
#define SPC_PSZ (32 * 10 + 4)
#define SPC_NBLK 16                                 // blocks per image

template <int CA>
__global__ void __launch_bounds__(256)
sp_wgrad_c1_kernel(const float* __restrict__ A, size_t a_stride, const float* __restrict__ B, size_t b_stride, int H, int W,
                   float* __restrict__ part) {
  __shared__ float red[256 * 10];
  const int tid = threadIdx.x, c = tid % CA, pl = tid / CA, NL = 256 / CA;
  const int b = blockIdx.y, Wp = W + 2, HWp = (H + 2) * Wp, P = H * W;
  A += (size_t)b * a_stride;
  B += (size_t)b * b_stride;
  const int per = (P + SPC_NBLK - 1) / SPC_NBLK, p0 = blockIdx.x * per, p1 = min(P, p0 + per);
  float acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.f;
  float bsum = 0.f;
  for (int p = p0 + pl; p < p1; p += NL) {
    const int y = p / W, x = p - y * W, o = (y + 1) * Wp + x + 1;
    const float a = CA == 1 ? A[o] : A[((size_t)(c >> 3) * HWp + o) * 8 + (c & 7)];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = fmaf(a, B[o + (t / 3 - 1) * Wp + (t % 3 - 1)], acc[t]);
    acc[9] += a;
    bsum += B[o];
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) red[tid * 10 + k] = acc[k];
  __syncthreads();
  float* out = part + ((size_t)b * gridDim.x + blockIdx.x) * SPC_PSZ;
  for (int i = tid; i < CA * 10; i += 256) {
    const int cc = i / 10, k = i - cc * 10;
    float s = 0.f;
    for (int l = 0; l < NL; ++l) s += red[(l * CA + cc) * 10 + k];
    out[cc * 10 + k] = s;
  }
  __syncthreads();
  red[tid] = c == 0 ? bsum : 0.f;                   // each pixel once: the channel-0 lanes
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int l = 0; l < NL; ++l) s += red[l * CA];
    out[CA * 10] = s;
  }
}

__global__ void __launch_bounds__(256)
sp_wgrad_c1_reduce_kernel(const float* __restrict__ part, int nblk, int ca, int bias_b, float* __restrict__ gw, float* __restrict__ gb) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int nbias = bias_b ? 1 : ca;
  if (e >= ca * 9 + nbias) return;
  const int o = e < ca * 9 ? (e / 9) * 10 + e % 9 : (bias_b ? ca * 10 : (e - ca * 9) * 10 + 9);
  float s = 0.f;
  for (int i = 0; i < nblk; ++i) s += part[(size_t)i * SPC_PSZ + o];
  if (e < ca * 9) gw[e] = s; else gb[e - ca * 9] = s;
}

int wgrad3x3_batched_ws_floats(int H, int W, int bs, int ca, int cb) {
  if (cb == 1) return bs * SPC_NBLK * SPC_PSZ;
  (void)H; (void)W; (void)ca;
  return 256 * SPW_PSZ;
}

int sp_wgrad_init() {
  static LdsOptinOnce once;
  return lds_optin(once, {{&sp_wgrad_mfma_kernel<64, 64>, SPW_MAX_SMEM}, {&sp_wgrad_mfma_kernel<64, 32>, SPW_MAX_SMEM},
                          {&sp_wgrad_mfma_kernel<32, 32>, SPW_MAX_SMEM}, {&sp_wgrad_mfma_kernel<32, 64>, SPW_MAX_SMEM}});
}

int wgrad3x3_batched(const float* A, size_t a_stride, const float* B, size_t b_stride, int bs, int H, int W, int ca, int cb,
                     int bias_b, float* ws, float* gw, float* gb, hipStream_t s) {
  if (!A || !B || !ws || !gw || !gb || bs < 1 || H < 1 || W < 1) return LEMO_ERR_ARG;
  if (cb == 1) {
    if (ca != 1 && ca != 32) return LEMO_ERR_SHAPE;
    const dim3 grid(SPC_NBLK, bs);
    if (ca == 1) hipLaunchKernelGGL(sp_wgrad_c1_kernel<1>, grid, dim3(256), 0, s, A, a_stride, B, b_stride, H, W, ws);
    else hipLaunchKernelGGL(sp_wgrad_c1_kernel<32>, grid, dim3(256), 0, s, A, a_stride, B, b_stride, H, W, ws);
    if (int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(sp_wgrad_c1_reduce_kernel, dim3((ca * 10 + 255) / 256), dim3(256), 0, s, ws, bs * SPC_NBLK, ca, bias_b, gw, gb);
    return (int)hipGetLastError();
  }
  if ((ca != 32 && ca != 64) || (cb != 32 && cb != 64) || spw_smem_bytes(W, ca, cb) > SPW_MAX_SMEM) return LEMO_ERR_SHAPE;
  if (int rc = sp_wgrad_init()) return rc;
  const int nwg = bs * H < 256 ? bs * H : 256;
  SpWgradArgs q{A, B, a_stride, b_stride, ws, bs, H, W, bias_b, nwg};
  const int smem = spw_smem_bytes(W, ca, cb), nout = 9 * ca * cb + 64;
#define SPW_GO(MA_, NB_)                                                                                              \
  hipLaunchKernelGGL((sp_wgrad_mfma_kernel<MA_, NB_>), dim3(nwg), dim3(256), smem, s, q);                            \
  if (int rc = (int)hipGetLastError()) return rc;                                                                    \
  hipLaunchKernelGGL((sp_wgrad_reduce_kernel<MA_, NB_>), dim3((nout + 255) / 256), dim3(256), 0, s, ws, nwg, bias_b, gw, gb)
  if (ca == 64 && cb == 64) { SPW_GO(64, 64); }
  else if (ca == 64) { SPW_GO(64, 32); }
  else if (cb == 64) { SPW_GO(32, 64); }
  else { SPW_GO(32, 32); }
#undef SPW_GO
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder end: dec_blc5 = deconv 32 -> 1 (+ bias, LeakyReLU), deconv 1 -> 1 (+ bias), then the L1 term
// ---------------------------------------------------------------------------------------------------------------------
// A stride-1 padding-1 ConvTranspose2d with weight w[nin][nout][3][3]: out[o][p] = sum_i sum_t in[i][p - off(t)] w[i][o][t],
// off(t) = (ky - 1, kx - 1); its adjoint: din[i][p] = sum_o sum_t dout[o][p + off(t)] w[i][o][t].  r1, rec, x0, drec, dpre8
// are plain padded images [(H+2)(W+2)] with a zero border; u / du the 32-channel CG8P input of dec_blc5.deconv1.
__global__ void __launch_bounds__(256)
sp_dec_end_fwd_kernel(const float* __restrict__ u, size_t u_stride, const float* __restrict__ w8, const float* __restrict__ b8,
                      float* __restrict__ r1, int H, int W) {
  const int Wp = W + 2, HWp = (H + 2) * Wp, p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  u += (size_t)b * u_stride;
  const int y = p / W, x = p - y * W, o = (y + 1) * Wp + x + 1;
  float a = 0.f;                                   // the order of conv3x3_c1_bwd_kernel (the same contraction)
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* qq = u + ((size_t)g * HWp + o - (t / 3 - 1) * Wp - (t % 3 - 1)) * 8;
      const float4 v0 = ld4(qq), v1 = ld4(qq + 4);
      const float* wc = w8 + (size_t)(g * 8) * 9 + t;
      a = fmaf(v0.x, wc[0], a); a = fmaf(v0.y, wc[9], a); a = fmaf(v0.z, wc[18], a); a = fmaf(v0.w, wc[27], a);
      a = fmaf(v1.x, wc[36], a); a = fmaf(v1.y, wc[45], a); a = fmaf(v1.z, wc[54], a); a = fmaf(v1.w, wc[63], a);
    }
  }
  r1[(size_t)b * HWp + o] = lrelu(a + b8[0]);
}

// rec = deconv(r1) + b9; L1 block partial of |rec - x|; drec = sign(rec - x) * gscale (null: evaluation); block (0, 0) thread 0
// advances Adam's step counter and bias corrections (ctr null: evaluation)
__global__ void __launch_bounds__(256)
sp_dec_end_loss_kernel(const float* __restrict__ r1, const float* __restrict__ w9, const float* __restrict__ b9,
                       const float* __restrict__ x0, float* __restrict__ rec, float* __restrict__ drec, float gscale,
                       float* __restrict__ lpart, float* __restrict__ ctr, double lr, int H, int W) {
  __shared__ float red[4];
  const int Wp = W + 2, HWp = (H + 2) * Wp, p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (ctr && p == 0 && b == 0) {
    int* ci = reinterpret_cast<int*>(ctr);
    const int step = ci[0] + 1;
    ci[0] = step;
    const AdamCoef ac = adam_coef_t(step, lr);
    ctr[1] = ac.neg_step;
    ctr[2] = ac.bc2s;
  }
  float ad = 0.f;
  if (p < H * W) {
    const size_t base = (size_t)b * HWp;
    const int y = p / W, x = p - y * W, o = (y + 1) * Wp + x + 1;
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) a = fmaf(r1[base + o - (t / 3 - 1) * Wp - (t % 3 - 1)], w9[t], a);
    const float rv = a + b9[0], d = x0 ? rv - x0[base + o] : 0.f;      // x0 null: the decoder's forward only
    rec[base + o] = rv;
    ad = fabsf(d);
    if (drec) drec[base + o] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * gscale;
  }
  if (!lpart) return;
  const float s = block_sum(ad, red);
  if (threadIdx.x == 0) lpart[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// dpre8 = (adjoint of the 1 -> 1 deconv applied to drec) * lrelu'(r1)
__global__ void __launch_bounds__(256)
sp_dec_end_bwd1_kernel(const float* __restrict__ drec, const float* __restrict__ w9, const float* __restrict__ r1,
                       float* __restrict__ dpre8, int H, int W) {
  const int Wp = W + 2, HWp = (H + 2) * Wp, p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  const size_t base = (size_t)b * HWp;
  const int y = p / W, x = p - y * W, o = (y + 1) * Wp + x + 1;
  float a = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) a = fmaf(drec[base + o + (t / 3 - 1) * Wp + (t % 3 - 1)], w9[t], a);
  dpre8[base + o] = a * lrelu_grad_from_out(r1[base + o]);
}

// du[i] = (adjoint of the 32 -> 1 deconv applied to dpre8)[i] * lrelu'(u[i]): one thread per (pixel, 8-channel group)
__global__ void __launch_bounds__(256)
sp_dec_end_bwd2_kernel(const float* __restrict__ dpre8, const float* __restrict__ w8, const float* __restrict__ u, size_t u_stride,
                       float* __restrict__ du, int H, int W) {
  const int Wp = W + 2, HWp = (H + 2) * Wp, P = H * W, b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 4 * P) return;
  const int g = idx / P, p = idx - g * P;
  const int y = p / W, x = p - y * W, o = (y + 1) * Wp + x + 1;
  const float* d8 = dpre8 + (size_t)b * HWp;
  float dv[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) dv[t] = d8[o + (t / 3 - 1) * Wp + (t % 3 - 1)];
  const size_t oo = (size_t)b * u_stride + ((size_t)g * HWp + o) * 8;
  float r[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float* wc = w8 + (size_t)(g * 8 + c) * 9;
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) a = fmaf(dv[t], wc[t], a);
    r[c] = a * lrelu_grad_from_out(u[oo + c]);
  }
  st4(du + oo, make_float4(r[0], r[1], r[2], r[3]));
  st4(du + oo + 4, make_float4(r[4], r[5], r[6], r[7]));
}

int dec_end_fwd(const float* u, size_t u_stride, const float* w8, const float* b8, const float* w9, const float* b9, float* r1,
                float* rec, const float* x0, float* drec, float gscale, float* lpart, float* ctr, double lr, int bs, int H, int W,
                hipStream_t s) {
  if (!u || !w8 || !b8 || !w9 || !b9 || !r1 || !rec || bs < 1 || H < 1 || W < 1) return LEMO_ERR_ARG;
  const dim3 grid((H * W + 255) / 256, bs);
  hipLaunchKernelGGL(sp_dec_end_fwd_kernel, grid, dim3(256), 0, s, u, u_stride, w8, b8, r1, H, W);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(sp_dec_end_loss_kernel, grid, dim3(256), 0, s, r1, w9, b9, x0, rec, drec, gscale, lpart, ctr, lr, H, W);
  return (int)hipGetLastError();
}
int dec_end_lpart_floats(int H, int W, int bs) { return bs * ((H * W + 255) / 256); }

int dec_end_bwd(const float* drec, const float* w9, const float* r1, float* dpre8, const float* w8, const float* u, size_t u_stride,
                float* du, int bs, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(sp_dec_end_bwd1_kernel, dim3((H * W + 255) / 256, bs), dim3(256), 0, s, drec, w9, r1, dpre8, H, W);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(sp_dec_end_bwd2_kernel, dim3((4 * H * W + 255) / 256, bs), dim3(256), 0, s, dpre8, w8, u, u_stride, du, H, W);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// small batched kernels: input padding, gradient sum, loss reduction, Adam, repack
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sp_pad_kernel(const float* __restrict__ x, float* __restrict__ x0, int H, int W) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, xx = p - y * W;
  x0[(size_t)b * (H + 2) * (W + 2) + (y + 1) * (W + 2) + xx + 1] = x[(size_t)b * H * W + p];
}

__global__ void __launch_bounds__(256)
sp_add_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 a = ld4(dst + 4 * i);
  const float4 c = ld4(src + 4 * i);
  a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
  st4(dst + 4 * i, a);
}

// losses[0] = sum(lpart) / n_rec, [1] = sum(spart) / n_smooth, [2] = w_rec [0] + w_smooth [1]; fixed-order f64 sums, one block
__global__ void __launch_bounds__(256)
sp_losses_kernel(const float* __restrict__ lpart, int nl, const float* __restrict__ spart, int ns, double n_rec, double n_smooth,
                 float w_rec, float w_smooth, float* __restrict__ losses) {
  __shared__ double red[2][256];
  double a = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nl; i += 256) a += (double)lpart[i];
  for (int i = threadIdx.x; i < ns; i += 256) c += (double)spart[i];
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) { red[0][threadIdx.x] += red[0][threadIdx.x + h]; red[1][threadIdx.x] += red[1][threadIdx.x + h]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float lr_ = (float)(red[0][0] / n_rec), ls = (float)(red[1][0] / n_smooth);
    losses[0] = lr_; losses[1] = ls; losses[2] = w_rec * lr_ + w_smooth * ls;
  }
}

__global__ void __launch_bounds__(256)
sp_adam_kernel(float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
               const float* __restrict__ ctr, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const AdamCoef ac{ctr[1], ctr[2]};
  float p = theta[i], mm = m[i], vv = v[i];
  adam_update_torch(p, mm, vv, g[i], ac);                     // common.hpp: torch.optim.Adam's evaluation order
  theta[i] = p; m[i] = mm; v[i] = vv;
}

// wt[tap][cin/8][cout][8] and wt2[cin/8][tap][cout][8] of the convolution Wc[co][ci][tap] with Wc = W (trans 0) or
// Wc[co][ci][tap] = W[ci][co][8 - tap] (trans 1: backward-data of a conv / forward of a transposed conv); W = [d0][d1][9] at src
__global__ void __launch_bounds__(256)
sp_repack_kernel(SpPackJobs J, const float* __restrict__ theta) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= J.total) return;
  int k = 0;
  while (k + 1 < J.n && idx >= J.j[k + 1].first) ++k;
  const SpPackJob& q = J.j[k];
  const int i = idx - q.first;
  const int e = i & 7, co = (i >> 3) % q.cout, r = (i >> 3) / q.cout;       // r = tap * (cin/8) + g
  const int ng = q.cin >> 3, tap = r / ng, g = r - tap * ng, ci = g * 8 + e;
  const float w = q.trans ? theta[q.src + ((size_t)ci * q.cout + co) * 9 + 8 - tap] : theta[q.src + ((size_t)co * q.cin + ci) * 9 + tap];
  q.wt[i] = w;
  q.wt2[(((size_t)g * 9 + tap) * q.cout + co) * 8 + e] = w;
}

int sp_repack(const SpPackJobs& J, const float* theta, hipStream_t s) {
  hipLaunchKernelGGL(sp_repack_kernel, dim3((J.total + 255) / 256), dim3(256), 0, s, J, theta);
  return (int)hipGetLastError();
}
int sp_pad(const float* x, float* x0, int bs, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(sp_pad_kernel, dim3((H * W + 255) / 256, bs), dim3(256), 0, s, x, x0, H, W);
  return (int)hipGetLastError();
}
int sp_add(float* dst, const float* src, size_t n, hipStream_t s) {
  const size_t n4 = n / 4;
  hipLaunchKernelGGL(sp_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dst, src, n4);
  return (int)hipGetLastError();
}
int sp_losses(const float* lpart, int nl, const float* spart, int ns, double n_rec, double n_smooth, float w_rec, float w_smooth,
              float* losses, hipStream_t s) {
  hipLaunchKernelGGL(sp_losses_kernel, dim3(1), dim3(256), 0, s, lpart, nl, spart, ns, n_rec, n_smooth, w_rec, w_smooth, losses);
  return (int)hipGetLastError();
}
int sp_adam(float* theta, float* m, float* v, const float* g, const float* ctr, int n, hipStream_t s) {
  hipLaunchKernelGGL(sp_adam_kernel, dim3((n + 255) / 256), dim3(256), 0, s, theta, m, v, g, ctr, n);
  return (int)hipGetLastError();
}

}  // namespace lemo
