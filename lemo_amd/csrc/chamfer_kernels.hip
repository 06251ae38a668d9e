// Batched brute-force nearest neighbour (the `chamfer` CUDA extension behind temp_prox/dist_chamfer.py:27,43) and the PROX
// scene-contact term's hot path (fitting_temp_slide.py:743-753): for every query point of xyz1 [B][N][3] the SQUARED distance to,
// and the index of, a nearest point of xyz2 [B or 1][M][3]; on request the same with the roles swapped.
//
// Distance.  d = (dx * dx + dy * dy) + dz * dz of the DIFFERENCES, as the extension computes it, never |a|^2 + |b|^2 - 2 a.b (its
// cancellation changes which neighbour wins).  The two additions are spelled as fmaf, so the host emulator and the device round alike.
// Ties go to the lowest index: targets are scanned in ascending order with a strict <, and partial results of target ranges are
// combined in ascending range order with a strict <.  Every pair is evaluated by the same three operations wherever it is scheduled,
// so a result does not depend on the number of ranges, bit for bit.
//
// Forward kernel.  256 threads; each lane keeps CH_QPT = 4 queries in registers, so a workgroup owns 1024 queries and every target
// fetched feeds four distance evaluations per lane.  Targets stream through LDS in chunks of CH_CHUNK = 512 as three arrays (x, y,
// z) and are read four at a time at a wave-uniform address (identical addresses broadcast: no bank conflicts).  Two LDS buffers:
// the next chunk's global loads are issued into registers before the current chunk's arithmetic and stored to the other buffer
// after it, one barrier per chunk.  2 x 3 x 512 x 4 B = 12 KB of static LDS.  Lanes past the end of a chunk see +inf coordinates:
// d = +inf never passes the strict <.
// A shared target set (B2 == 1) is never copied: the batch is flattened into one query list of B N points.
// When there are too few query workgroups to fill the chip, grid.y splits the target range; each split writes its (dist, idx) to
// the caller's workspace and chamfer_combine_kernel folds them.  fp32 VALU only: per pair 3 subtractions, 1 multiply, 2 fused
// multiply-adds, 1 compare and 2 selects; there is no matrix-core form of an arg-min.
//
// Masked form (chamfer_masked_forward: the scan-to-mesh / mesh-to-scan terms of fitting_temp_slide.py:657-667, where every frame has
// its own number of valid scan points and its own visible vertices).  The same kernel, instantiated with MASKED: an invalid target is
// staged into LDS as +inf coordinates, exactly like the lanes past the end of a chunk, so it never passes the strict <; valid means
// index < n[b] (where a count is given) AND mask[b][index] != 0 (where a mask is given).  Indices refer to the original arrays.  An
// invalid query, and every query of an entry without a valid target, reports dist = 0 and idx = -1, which the backward kernels already
// read as "no gradient".  Nothing is compacted and nothing waits for the device.  Everything above carries over: the same three
// operations per pair, lowest index on ties among the valid targets, the same bits for every split count.
//
// Backward, as the extension defines it: grad1[i] = 2 g1[i] (x1[i] - x2[idx1[i]]) + sum_{j: idx2[j] = i} 2 g2[j] (x1[i] - x2[j]) and the
// mirror image.  The own-side term is a plain store (or a memset where that direction was not computed); the scattered term is an fp32
// atomicAdd, launched after the stores.  A side whose gradient pointer is NULL is neither computed nor written.
#include "kernels.hpp"

#include <algorithm>

namespace lemo {

#define CH_BLOCK 256
#define CH_QPT 4
#define CH_QPW (CH_BLOCK * CH_QPT)                           // queries per workgroup
#define CH_CHUNK 512                                         // targets per LDS buffer
#define CH_SPLIT_MIN 1024                                    // an automatic split never holds fewer targets than this
#define CH_TARGET_WGS 1024                                   // workgroups wanted before the target range stops being split (4 per CU)
#define CH_MAX_SPLITS 1024

struct ChMask {                                              // MASKED only; any of the four may be NULL
  const int* n1; const unsigned char* qm;                    // valid leading queries [B], query mask [B][N]
  const int* n2; const unsigned char* tm;                    // valid leading targets [B], target mask [B][M]
  int fin;                                                   // this launch writes the final result (no combine follows)
};

__device__ __forceinline__ bool ch_query_valid(const ChMask& mk, int b, int N, int i) {
  return (!mk.n1 || i < mk.n1[b]) && (!mk.qm || mk.qm[(size_t)b * N + i] != 0);
}

// queries q of [0, N) against targets [t0, t1) of one batch entry; grid (query block, split, batch)
template <bool MASKED>
__global__ void __launch_bounds__(CH_BLOCK) chamfer_nn_kernel(const float* __restrict__ xq, const float* __restrict__ xt, int N, int M,
                                                              long long tstride, int split_len, float* __restrict__ dist,
                                                              int* __restrict__ idx, long long ostride, ChMask mk) {
  __shared__ __attribute__((aligned(16))) float sx[2][CH_CHUNK];
  __shared__ __attribute__((aligned(16))) float sy[2][CH_CHUNK];
  __shared__ __attribute__((aligned(16))) float sz[2][CH_CHUNK];
  const int tid = threadIdx.x, b = blockIdx.z, sp = blockIdx.y;
  const int t0 = sp * split_len;
  int t1 = min(M, t0 + split_len);
  if constexpr (MASKED) {                                    // targets past the count are invalid: the range ends there; a workgroup
    if (mk.n2) t1 = min(t1, mk.n2[b]);                       // whose queries all lie past the count scans nothing (uniform)
    if (mk.n1 && (int)(blockIdx.x * CH_QPW) >= mk.n1[b]) t1 = t0;
  }
  const float* __restrict__ q = xq + (size_t)b * N * 3;
  const float* __restrict__ t = xt + (size_t)b * tstride;
  const int q0 = blockIdx.x * CH_QPW + tid;

  float qx[CH_QPT], qy[CH_QPT], qz[CH_QPT], best[CH_QPT];
  int bi[CH_QPT];
#pragma unroll
  for (int k = 0; k < CH_QPT; ++k) {
    const int i = min(q0 + k * CH_BLOCK, N - 1);             // lanes past the end repeat the last query and do not store
    qx[k] = q[3 * (size_t)i]; qy[k] = q[3 * (size_t)i + 1]; qz[k] = q[3 * (size_t)i + 2];
    best[k] = INFINITY; bi[k] = t0;
  }

  // a chunk is 3 * CH_CHUNK consecutive floats of the target array: 6 per thread, coalesced
  constexpr int PER = 3 * CH_CHUNK / CH_BLOCK;
  float stage[PER];
  auto fetch = [&](int c0) {
    const size_t base = 3 * (size_t)c0;
    const int lim = 3 * min(t1 - c0, CH_CHUNK);              // floats of this chunk that exist
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int e = tid + r * CH_BLOCK;
      bool ok = e < lim;
      if constexpr (MASKED) ok = ok && (!mk.tm || mk.tm[(size_t)b * M + c0 + e / 3] != 0);
      stage[r] = ok ? t[base + e] : INFINITY;
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int e = tid + r * CH_BLOCK, p = e / 3, c = e - 3 * p;
      float* dst = c == 0 ? sx[buf] : (c == 1 ? sy[buf] : sz[buf]);
      dst[p] = stage[r];
    }
  };

  fetch(t0);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int c0 = t0; c0 < t1; c0 += CH_CHUNK, buf ^= 1) {
    const bool more = c0 + CH_CHUNK < t1;
    if (more) fetch(c0 + CH_CHUNK);
    const int cnt = min(CH_CHUNK, t1 - c0), cnt4 = (cnt + 3) & ~3;
    for (int j = 0; j < cnt4; j += 4) {
      const float4 X = *reinterpret_cast<const float4*>(&sx[buf][j]);
      const float4 Y = *reinterpret_cast<const float4*>(&sy[buf][j]);
      const float4 Z = *reinterpret_cast<const float4*>(&sz[buf][j]);
      const float tx[4] = {X.x, X.y, X.z, X.w}, ty[4] = {Y.x, Y.y, Y.z, Y.w}, tz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jj = c0 + j + u;
#pragma unroll
        for (int k = 0; k < CH_QPT; ++k) {
          const float dx = qx[k] - tx[u], dy = qy[k] - ty[u], dz = qz[k] - tz[u];
          const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          const bool lt = d < best[k];
          best[k] = lt ? d : best[k];
          bi[k] = lt ? jj : bi[k];
        }
      }
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }

  float* __restrict__ od = dist + (size_t)sp * ostride + (size_t)b * N;
  int* __restrict__ oi = idx + (size_t)sp * ostride + (size_t)b * N;
#pragma unroll
  for (int k = 0; k < CH_QPT; ++k) {
    const int i = q0 + k * CH_BLOCK;
    if (i >= N) continue;
    if constexpr (MASKED) {
      if (mk.fin && (!(best[k] < INFINITY) || !ch_query_valid(mk, b, N, i))) { od[i] = 0.f; oi[i] = -1; continue; }
    }
    od[i] = best[k]; oi[i] = bi[k];
  }
}

// fold S partial results [S][n] in ascending split order: a later split wins only with a strictly smaller distance
template <bool MASKED>
__global__ void __launch_bounds__(CH_BLOCK) chamfer_combine_kernel(const float* __restrict__ pd, const int* __restrict__ pi, int S,
                                                                   long long n, float* __restrict__ dist, int* __restrict__ idx, int N,
                                                                   ChMask mk) {
  const long long i = (long long)blockIdx.x * CH_BLOCK + threadIdx.x;
  if (i >= n) return;
  if constexpr (MASKED) {                                    // the partial results of an invalid query are never read
    if (!ch_query_valid(mk, (int)(i / N), N, (int)(i % N))) { dist[i] = 0.f; idx[i] = -1; return; }
  }
  float best = pd[i];
  int bi = pi[i];
  for (int s = 1; s < S; ++s) {
    const float d = pd[(size_t)s * n + i];
    const int j = pi[(size_t)s * n + i];
    if (d < best) { best = d; bi = j; }
  }
  if constexpr (MASKED) {
    if (!(best < INFINITY)) { best = 0.f; bi = -1; }          // no valid target in any range
  }
  dist[i] = best;
  idx[i] = bi;
}

// own-side term: ga[b][i] = 2 g[b][i] (xa[b][i] - xb[b][idx[b][i]]); grid over B N elements, batch b = i / N
__global__ void __launch_bounds__(CH_BLOCK) chamfer_bwd_own_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                   const float* __restrict__ g, const int* __restrict__ idx, long long n,
                                                                   int N, int M, long long bstride, float* __restrict__ ga) {
  const long long i = (long long)blockIdx.x * CH_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int j = idx[i];
  if (j < 0 || j >= M) { ga[3 * i] = 0.f; ga[3 * i + 1] = 0.f; ga[3 * i + 2] = 0.f; return; }      // not an index this library wrote
  const float* __restrict__ p = xb + (size_t)(i / N) * bstride + 3 * (size_t)j;
  const float w = 2.0f * g[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) ga[3 * i + c] = w * (xa[3 * i + c] - p[c]);
}

// scattered term: gb[b][idx[b][i]] -= 2 g[b][i] (xa[b][i] - xb[b][idx[b][i]])
__global__ void __launch_bounds__(CH_BLOCK) chamfer_bwd_scatter_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                       const float* __restrict__ g, const int* __restrict__ idx, long long n,
                                                                       int N, int M, long long bstride, float* __restrict__ gb) {
  const long long i = (long long)blockIdx.x * CH_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int j = idx[i];
  if (j < 0 || j >= M) return;
  const size_t o = (size_t)(i / N) * bstride + 3 * (size_t)j;
  const float w = 2.0f * g[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(&gb[o + c], -(w * (xa[3 * i + c] - xb[o + c])));
}

namespace {

struct ChShape { int B, N, M, shared, reverse; };

int ch_shape(int B, int N, int M, int flags, ChShape& s) {
  if (flags & ~(LEMO_CHAMFER_SHARED | LEMO_CHAMFER_REVERSE)) return LEMO_ERR_ARG;
  s.shared = (flags & LEMO_CHAMFER_SHARED) ? 1 : 0;
  s.reverse = (flags & LEMO_CHAMFER_REVERSE) ? 1 : 0;
  if (s.shared && s.reverse) return LEMO_ERR_ARG;            // the reverse direction is not defined for a shared target set
  if (B < 1 || N < 1 || M < 1 || B > 65535) return LEMO_ERR_SHAPE;
  if ((long long)B * N > (1ll << 30) || (long long)B * M > (1ll << 30)) return LEMO_ERR_SHAPE;
  s.B = B; s.N = N; s.M = M;
  return 0;
}

// targets per split for Bq batch entries of Nq queries against Mt targets; the split count is ceil(Mt / length)
int ch_split_len(int Bq, int Nq, int Mt, int split) {
  int S;
  if (split > 0) {
    S = std::min(std::min(split, Mt), CH_MAX_SPLITS);
  } else {
    const long long wgs = (long long)Bq * ((Nq + CH_QPW - 1) / CH_QPW);
    const long long want = (CH_TARGET_WGS + wgs - 1) / wgs;
    S = (int)std::max(1ll, std::min(std::min(want, (long long)(Mt / CH_SPLIT_MIN)), (long long)CH_MAX_SPLITS));
  }
  return (Mt + S - 1) / S;
}

long long ch_ws_elems(int Bq, int Nq, int Mt, int split) {
  const int len = ch_split_len(Bq, Nq, Mt, split);
  const int S = (Mt + len - 1) / len;
  return S > 1 ? (long long)S * Bq * Nq : 0;
}

template <bool MASKED>
int ch_nn(const float* xq, const float* xt, int Bq, int Nq, int Mt, long long tstride, int split, float* dist, int* idx, void* ws,
          long long ws_bytes, hipStream_t s, ChMask mk = ChMask{nullptr, nullptr, nullptr, nullptr, 0}) {
  const int len = ch_split_len(Bq, Nq, Mt, split);
  const int S = (Mt + len - 1) / len;
  const long long n = (long long)Bq * Nq;
  const dim3 grid((Nq + CH_QPW - 1) / CH_QPW, S, Bq);
  if (S == 1) {
    mk.fin = 1;
    hipLaunchKernelGGL((chamfer_nn_kernel<MASKED>), grid, dim3(CH_BLOCK), 0, s, xq, xt, Nq, Mt, tstride, len, dist, idx, 0ll, mk);
    return (int)hipGetLastError();
  }
  if (!ws || ws_bytes < (long long)S * n * 8) return LEMO_ERR_ARG;
  float* pd = static_cast<float*>(ws);
  int* pi = reinterpret_cast<int*>(pd + (size_t)S * n);
  mk.fin = 0;
  hipLaunchKernelGGL((chamfer_nn_kernel<MASKED>), grid, dim3(CH_BLOCK), 0, s, xq, xt, Nq, Mt, tstride, len, pd, pi, n, mk);
  hipLaunchKernelGGL((chamfer_combine_kernel<MASKED>), dim3((unsigned)((n + CH_BLOCK - 1) / CH_BLOCK)), dim3(CH_BLOCK), 0, s, pd, pi, S, n, dist,
                     idx, Nq, mk);
  return (int)hipGetLastError();
}

}  // namespace

long long chamfer_workspace_bytes(int B, int N, int M, int flags, int split) {
  ChShape c;
  if (ch_shape(B, N, M, flags, c) || split < 0) return -1;
  long long e = c.shared ? ch_ws_elems(1, B * N, M, split) : ch_ws_elems(B, N, M, split);
  if (c.reverse) e = std::max(e, ch_ws_elems(B, M, N, split));
  return e * 8;
}

int chamfer_forward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, int split, float* dist1, int* idx1,
                    float* dist2, int* idx2, void* ws, long long ws_bytes, hipStream_t s) {
  ChShape c;
  if (int e = ch_shape(B, N, M, flags, c)) return e;
  if (!xyz1 || !xyz2 || !dist1 || !idx1 || split < 0 || ws_bytes < 0) return LEMO_ERR_ARG;
  if (c.reverse && (!dist2 || !idx2)) return LEMO_ERR_ARG;
  int e = c.shared ? ch_nn<false>(xyz1, xyz2, 1, B * N, M, 0, split, dist1, idx1, ws, ws_bytes, s)
                   : ch_nn<false>(xyz1, xyz2, B, N, M, 3ll * M, split, dist1, idx1, ws, ws_bytes, s);
  if (e || !c.reverse) return e;
  return ch_nn<false>(xyz2, xyz1, B, M, N, 3ll * N, split, dist2, idx2, ws, ws_bytes, s);        // the workspace is reused in stream order
}

int chamfer_masked_forward(const float* xyz1, const float* xyz2, int B, int N, int M, const int* n1, const unsigned char* q_mask,
                           const int* n2, const unsigned char* t_mask, int split, float* dist1, int* idx1, void* ws, long long ws_bytes,
                           hipStream_t s) {
  ChShape c;
  if (int e = ch_shape(B, N, M, 0, c)) return e;
  if (!xyz1 || !xyz2 || !dist1 || !idx1 || split < 0 || ws_bytes < 0) return LEMO_ERR_ARG;
  return ch_nn<true>(xyz1, xyz2, B, N, M, 3ll * M, split, dist1, idx1, ws, ws_bytes, s, ChMask{n1, q_mask, n2, t_mask, 0});
}

int chamfer_backward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, const float* g1, const int* idx1,
                     const float* g2, const int* idx2, float* grad1, float* grad2, hipStream_t s) {
  ChShape c;
  if (int e = ch_shape(B, N, M, flags, c)) return e;
  if (!xyz1 || !xyz2 || !g1 || !idx1) return LEMO_ERR_ARG;
  if (c.reverse && (!g2 || !idx2)) return LEMO_ERR_ARG;
  if (!grad1 && !grad2) return 0;
  const long long n1 = (long long)B * N, n2 = (long long)B * M;                       // side 2 has n2 elements only when it is not shared
  const long long st2 = c.shared ? 0 : 3ll * M, st1 = 3ll * N;
  const dim3 blk(CH_BLOCK), g_1((unsigned)((n1 + CH_BLOCK - 1) / CH_BLOCK)), g_2((unsigned)((n2 + CH_BLOCK - 1) / CH_BLOCK));
  // own-side terms first (plain stores), the scattered terms after them in stream order
  if (grad1) hipLaunchKernelGGL(chamfer_bwd_own_kernel, g_1, blk, 0, s, xyz1, xyz2, g1, idx1, n1, N, M, st2, grad1);
  if (grad2) {
    if (c.reverse) {
      hipLaunchKernelGGL(chamfer_bwd_own_kernel, g_2, blk, 0, s, xyz2, xyz1, g2, idx2, n2, M, N, st1, grad2);
    } else if (hipError_t e = hipMemsetAsync(grad2, 0, (size_t)(c.shared ? 1 : B) * M * 3 * sizeof(float), s)) {
      return (int)e;
    }
    hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, g_1, blk, 0, s, xyz1, xyz2, g1, idx1, n1, N, M, st2, grad2);
  }
  if (grad1 && c.reverse) hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, g_2, blk, 0, s, xyz2, xyz1, g2, idx2, n2, M, N, st1, grad1);
  return (int)hipGetLastError();
}

void chamfer_sizes(int* out) {
  out[0] = CH_QPW; out[1] = CH_CHUNK; out[2] = CH_SPLIT_MIN; out[3] = CH_TARGET_WGS;
}

}  // namespace lemo

extern "C" {
long long lemo_chamfer_workspace_bytes(int B, int N, int M, int flags, int split) {
  return lemo::chamfer_workspace_bytes(B, N, M, flags, split);
}
int lemo_chamfer_forward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, int split, float* dist1, int* idx1,
                         float* dist2, int* idx2, void* ws, long long ws_bytes, void* stream) {
  return lemo::chamfer_forward(xyz1, xyz2, B, N, M, flags, split, dist1, idx1, dist2, idx2, ws, ws_bytes, (hipStream_t)stream);
}
int lemo_chamfer_backward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, const float* g1, const int* idx1,
                          const float* g2, const int* idx2, float* grad1, float* grad2, void* stream) {
  return lemo::chamfer_backward(xyz1, xyz2, B, N, M, flags, g1, idx1, g2, idx2, grad1, grad2, (hipStream_t)stream);
}
void lemo_chamfer_sizes(int* out4) { lemo::chamfer_sizes(out4); }
int lemo_chamfer_masked_forward(const float* xyz1, const float* xyz2, int B, int N, int M, const int* n1, const unsigned char* q_mask,
                                const int* n2, const unsigned char* t_mask, int split, float* dist1, int* idx1, void* ws, long long ws_bytes,
                                void* stream) {
  return lemo::chamfer_masked_forward(xyz1, xyz2, B, N, M, n1, q_mask, n2, t_mask, split, dist1, idx1, ws, ws_bytes, (hipStream_t)stream);
}
}  // extern "C"
