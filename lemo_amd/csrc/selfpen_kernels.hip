// The self-penetration term of SMPLifyLoss on the device (fitting_temp_slide.py:618-635, fit_temp_loadprox_slide.py:314-344): the three
// pieces the reference takes from the `mesh_intersection` package (torch-mesh-isect) -- BVH collision search, FilterFaces and
// DistanceFieldPenetrationLoss -- for B frames at once.  That package is not part of this project's environment: the behaviour below
// follows the published cone distance field (Tzionas et al., IJCV 2016, as used by SMPLify-X) and the package's documented interface,
// NOT a run of it; bit or ulp conformance to it is unverified.
//
// 1. Search.  Triangles i < j of one frame COLLIDE iff
//      (a) both are valid: every vertex index in [0, V), every coordinate finite;
//      (b) they share no vertex index;
//      (c) their axis-aligned boxes overlap (min / max of the fp32 coordinates, compared exactly: true for every pair that meets in
//          exact arithmetic, so it removes nothing from the definition, and it is the same test in every mode);
//      (d) an edge of one meets the other: six segment / triangle tests by Moeller-Trumbore, the rule of visibility_kernels.hip --
//          inclusive on every bound, either side counts, det == 0 (parallel, degenerate, coplanar) or NaN never hits;
//      (e) with a segmentation, none of segm[i] == segm[j], parents[i] == segm[j], parents[j] == segm[i], ign[segm[i]][segm[j]],
//          ign[segm[j]][segm[i]] (FilterFaces, folded in).
//    fp32 VALU only, explicit fmaf chains, contraction off: sp_collide(i, j) is ONE function of the pair, so the set of pairs does not
//    depend on who enumerates the candidates.  Output: pairs [B][C][2] in lexicographic order, -1 behind the last, the first C on
//    overflow, and count [B] = the true number (saturating at 2^31 - 1).  No order depends on an atomic:
//      count pass  : cnt[i] = number of j > i that collide with i                                   (one thread per face)
//      sp_scan     : exclusive prefix sum per frame -> off[i] (clamped to C), count[b], the -1 tail  (one workgroup per frame)
//      fill pass   : the same enumeration again; face i owns pairs[off[i] .. off[i] + min(cnt[i], C - off[i])) and keeps it sorted by j
//                    with an insertion (the candidates of the grid arrive in cell order; in brute force j ascends and it appends).
//                    A face without a collision, or behind the capacity, leaves at once.
//    BRUTE: chamfer_nn_kernel's structure -- 256 faces per workgroup in registers, the boxes of the faces j streamed through LDS in
//    chunks of 256 as six arrays read at a wave-uniform address (a broadcast, no bank conflict), two buffers, one barrier per chunk,
//    12 KB of static LDS; only chunks at or behind the workgroup's own faces are visited.  The box reject is the hot loop (2.2e8 per
//    frame at the PROX shape); the narrow phase runs behind it for the few pairs that survive.
//    GRID: sp_bin_kernel (one workgroup per frame) bins every valid face by the cell of its box's MIN corner in a G x G x G grid over
//    the frame's bounding box (counting sort in LDS, G <= 16: 16 KB of counters), and records K = the largest number of cells a box
//    spans per axis.  grid_cell (geom_device.hpp) is monotone, so a face j whose box overlaps that of i has cell(min_j) in
//    [cell(min_i) - K, cell(max_i)] on every axis: integer logic, exact, nothing is inflated by a tolerance.  The query visits those
//    cells (the cells of one x-row are contiguous) and reads the candidates' boxes in cell order.
// 2. Loss.  Triangle f = (p0, p1, p2): unit normal n, circumcentre o (barycentric form), circumradius r = abc / (2 |e1 x e2|).  Point v:
//    h = n . (v - o), rho = |(v - o) - h n|, Phi = rho / (r - (r / sigma) h), Upsilon(h) = -h + 1 - sigma (h <= -sigma),
//    -(1 - 2 sigma) / (4 sigma^2) h^2 - h / (2 sigma) + (3 - 2 sigma) / 4 (|h| < sigma), 0 (h >= sigma, and h > 0 without
//    penalize_outside); Psi_f(v) = (1 - Phi) Upsilon(h) where Phi < 1 and the denominator is positive, else 0.
//    L[b] = sum over the listed pairs (i, j) of sum_{v in j} Psi_i(v)^2 + sum_{v in i} Psi_j(v)^2.
//    Everything is evaluated RELATIVE TO p0 (q1 = p1 - p0, q2 = p2 - p0, x = v - p0): a body stands 3 m from the camera and its
//    triangles are 1 cm wide, and a circumcentre formed in camera coordinates would carry 3e-7 m of rounding into an h of 1e-3 m.
//    Forward: one workgroup per frame, a fixed-order tree sum (deterministic).  Backward: the full gradient -- through the point and
//    through n, o, r of the receiving triangle.  d Psi / d(n, o, r, x) is written out by hand (sp_psi); the Jacobian of (n, o, r) with
//    respect to (q1, q2) comes from evaluating the SAME templated setup (sp_cone) on forward-mode duals with six partials, once per
//    triangle and shared by its three points; d/dp0 = -(d/dq1 + d/dq2 + sum d/dx).  Scatter by fp32 atomicAdd, as lemo_chamfer_backward.
//    A zero-area triangle contributes nothing and receives nothing; an empty list gives L = 0 and a zero gradient without a host test.
// AUTO: see SP_AUTO_MODE below.
#include "geom_device.hpp"
#include "fixed_acc.hpp"
#include "kernels.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace lemo {

#define SP_BLOCK 256
#define SP_GMAX 16                                           // largest (and default) grid side: G^3 counters in LDS
#define SP_HDR 16                                            // 4-byte words of a frame's grid header
#define SP_PMAX 64                                           // largest side of the ignore table

struct SpFace { int id[3]; float p[3][3]; float lo[3], hi[3]; bool ok; };

// face f of the frame; not ok (an index outside [0, V), a coordinate that is not finite): an empty box, which overlaps nothing
__device__ __forceinline__ void sp_face(const float* __restrict__ vf, int V, const int* __restrict__ faces, int f, SpFace& t) {
  const bool ids = face_ids(faces, f, V, t.id);
  const bool ok = face_corners(vf, t.id, ids, t.p);
  t.ok = ok;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t.lo[a] = ok ? fminf(t.p[0][a], fminf(t.p[1][a], t.p[2][a])) : GEOM_FMAX;
    t.hi[a] = ok ? fmaxf(t.p[0][a], fmaxf(t.p[1][a], t.p[2][a])) : -GEOM_FMAX;
  }
}

__device__ __forceinline__ bool sp_overlap(const float lo[3], const float hi[3], float l0, float l1, float l2, float h0, float h1, float h2) {
  return lo[0] <= h0 && l0 <= hi[0] && lo[1] <= h1 && l1 <= hi[1] && lo[2] <= h2 && l2 <= hi[2];
}

// the segment a -> b against the triangle (v0; e1, e2): Moeller-Trumbore without a division, inclusive, either side, det == 0: no hit
__device__ __forceinline__ bool sp_seg_tri(const float a[3], const float b[3], const float v0[3], const float e1[3], const float e2[3]) {
  const float d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float tv[3] = {a[0] - v0[0], a[1] - v0[1], a[2] - v0[2]};
  float pv[3], qv[3];
  cross3(d, e2, pv);
  cross3(tv, e1, qv);
  const float det = dot3(e1, pv), U = dot3(tv, pv), W = dot3(d, qv), T = dot3(e2, qv), S = U + W;
  const bool pos = det > 0.f && U >= 0.f && W >= 0.f && S <= det && T >= 0.f && T <= det;
  const bool neg = det < 0.f && U <= 0.f && W <= 0.f && S >= det && T <= 0.f && T >= det;
  return pos || neg;
}

struct SpSegm { const int* segm; const int* parents; const unsigned char* ign; int P; };

__device__ __forceinline__ bool sp_filtered(const SpSegm& g, int i, int j) {
  if (!g.segm) return false;
  const int si = g.segm[i], sj = g.segm[j];
  if (si == sj) return true;
  if (g.parents && (g.parents[i] == sj || g.parents[j] == si)) return true;
  if (g.ign && (unsigned)si < (unsigned)g.P && (unsigned)sj < (unsigned)g.P && (g.ign[si * g.P + sj] || g.ign[sj * g.P + si])) return true;
  return false;
}

// rules (b), (d), (e) for valid faces A = face i and Bf = face j, i < j, whose boxes overlap
__device__ __forceinline__ bool sp_collide(const SpFace& A, const SpFace& Bf, const SpSegm& g, int i, int j) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (A.id[k] == Bf.id[0] || A.id[k] == Bf.id[1] || A.id[k] == Bf.id[2]) return false;
  if (sp_filtered(g, i, j)) return false;
  float a1[3], a2[3], b1[3], b2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a1[k] = A.p[1][k] - A.p[0][k]; a2[k] = A.p[2][k] - A.p[0][k];
    b1[k] = Bf.p[1][k] - Bf.p[0][k]; b2[k] = Bf.p[2][k] - Bf.p[0][k];
  }
  return sp_seg_tri(A.p[0], A.p[1], Bf.p[0], b1, b2) || sp_seg_tri(A.p[1], A.p[2], Bf.p[0], b1, b2) || sp_seg_tri(A.p[2], A.p[0], Bf.p[0], b1, b2) ||
         sp_seg_tri(Bf.p[0], Bf.p[1], A.p[0], a1, a2) || sp_seg_tri(Bf.p[1], Bf.p[2], A.p[0], a1, a2) || sp_seg_tri(Bf.p[2], Bf.p[0], A.p[0], a1, a2);
}

// face i's slice pr[0 .. m) of the pair list, sorted by j; holds `filled` entries.  Keeps the m smallest j.
__device__ __forceinline__ void sp_insert(int* __restrict__ pr, int m, int& filled, int i, int j) {
  int k = filled;
  if (k == m) {
    if (j >= pr[2 * (m - 1) + 1]) return;
    k = m - 1;
  } else {
    pr[2 * k] = i;
    ++filled;
  }
  while (k > 0 && pr[2 * (k - 1) + 1] > j) { pr[2 * k + 1] = pr[2 * (k - 1) + 1]; --k; }
  pr[2 * k + 1] = j;
}

// A frame's workspace, laid out from `frame`: cnt [F], off [F]; GRID adds hdr [SP_HDR] ([0..2] x0, [3..5] scale as float bits,
// [6..8] K), cell_start [G^3 + 1], item [F], box [F][6] (floats, in cell order).  P is a pointer to 4-byte words in the kernels, and
// long long on the host, where laying a frame out from word 0 gives its size as `end`.
template <typename P> struct SpWs { P cnt, off, hdr, cell_start, item, box, end; };
template <typename P> __host__ __device__ inline SpWs<P> sp_ws(P frame, int F, int G, int mode) {
  SpWs<P> w = {};
  w.cnt = frame; w.off = w.cnt + F; w.end = w.off + F;
  if (mode == LEMO_SELFPEN_GRID) {
    w.hdr = w.end; w.cell_start = w.hdr + SP_HDR; w.item = w.cell_start + (G * G * G + 1); w.box = w.item + F; w.end = w.box + 6ll * F;
  }
  return w;
}

// what a thread of a fill pass owns: -> m (0: nothing to do)
__device__ __forceinline__ int sp_slice(const int* __restrict__ cnt, const int* __restrict__ off, int i, int F, int C, int& base) {
  base = 0;
  if (i >= F) return 0;
  base = off[i];
  return max(0, min(cnt[i], C - base));
}

// ---- brute force -------------------------------------------------------------------------------------------------------------
// grid (face block, frame)
template <bool FILL>
__global__ void __launch_bounds__(SP_BLOCK) sp_brute_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F, SpSegm g,
                                                             int* __restrict__ ws, long long wstride, int* __restrict__ pairs, int C) {
  __shared__ __attribute__((aligned(16))) float sb[2][6][SP_BLOCK];
  __shared__ int s_any;
  const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x * SP_BLOCK + tid;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const SpWs<int*> w = sp_ws(ws + (size_t)b * wstride, F, 0, LEMO_SELFPEN_BRUTE);
  int m = 0, base = 0, filled = 0, found = 0;
  if (FILL) {
    m = sp_slice(w.cnt, w.off, i, F, C, base);
    if (tid == 0) s_any = 0;
    __syncthreads();
    if (m > 0) s_any = 1;
    __syncthreads();
    if (!s_any) return;                                       // uniform: no face of this workgroup has a pair to write
  }
  int* __restrict__ pr = pairs + ((size_t)b * C + base) * 2;
  SpFace me;
  if (i < F) {
    sp_face(vf, V, faces, i, me);
  } else {
    me.ok = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) { me.lo[a] = GEOM_FMAX; me.hi[a] = -GEOM_FMAX; }
  }
  const bool active = FILL ? m > 0 : true;

  float stage[6];
  auto fetch = [&](int c0) {
    const int f = c0 + tid;
    if (f < F) {
      SpFace t;
      sp_face(vf, V, faces, f, t);
#pragma unroll
      for (int a = 0; a < 3; ++a) { stage[a] = t.lo[a]; stage[3 + a] = t.hi[a]; }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) { stage[a] = GEOM_FMAX; stage[3 + a] = -GEOM_FMAX; }
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int a = 0; a < 6; ++a) sb[buf][a][tid] = stage[a];
  };

  const int first = blockIdx.x * SP_BLOCK;                    // j > i: nothing in front of the workgroup's own faces
  fetch(first);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int c0 = first; c0 < F; c0 += SP_BLOCK, buf ^= 1) {
    const bool more = c0 + SP_BLOCK < F;
    if (more) fetch(c0 + SP_BLOCK);
    const int n = min(SP_BLOCK, F - c0);
    if (active) {
      for (int jj = 0; jj < n; ++jj) {
        const int j = c0 + jj;
        if (j > i && sp_overlap(me.lo, me.hi, sb[buf][0][jj], sb[buf][1][jj], sb[buf][2][jj], sb[buf][3][jj], sb[buf][4][jj], sb[buf][5][jj])) {
          SpFace other;
          sp_face(vf, V, faces, j, other);
          if (sp_collide(me, other, g, i, j)) {
            if (FILL) sp_insert(pr, m, filled, i, j); else ++found;
          }
        }
      }
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }
  if (!FILL && i < F) w.cnt[i] = found;
}

// ---- per-frame prefix sum ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_BLOCK) sp_scan_kernel(int F, int* __restrict__ ws, long long wstride, int* __restrict__ pairs, int C,
                                                            int* __restrict__ count) {
  __shared__ long long s_part[SP_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x;
  const SpWs<int*> w = sp_ws(ws + (size_t)b * wstride, F, 0, LEMO_SELFPEN_BRUTE);
  const long long total = block_exclusive_scan<SP_BLOCK>(F, s_part, [&](int k) { return w.cnt[k]; },
                                                         [&](int k, long long acc) { w.off[k] = (int)(acc < (long long)C ? acc : (long long)C); });
  if (tid == 0) count[b] = (int)(total < 2147483647ll ? total : 2147483647ll);
  int* __restrict__ pb = pairs + (size_t)b * C * 2;
  for (long long c = (total < (long long)C ? total : (long long)C) + tid; c < C; c += SP_BLOCK) { pb[2 * c] = -1; pb[2 * c + 1] = -1; }
}

// ---- grid ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_BLOCK) sp_bin_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F, int G,
                                                           int* __restrict__ ws, long long wstride) {
  __shared__ unsigned s_box[6];                                // max keys of hi[a] and of -lo[a]
  __shared__ unsigned s_k[3];
  __shared__ int s_cnt[SP_GMAX * SP_GMAX * SP_GMAX];
  __shared__ int s_part[SP_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x, nc = G * G * G;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const SpWs<int*> w = sp_ws(ws + (size_t)b * wstride, F, G, LEMO_SELFPEN_GRID);
  float* __restrict__ box = reinterpret_cast<float*>(w.box);
  if (tid < 6) s_box[tid] = 0u;
  if (tid < 3) s_k[tid] = 0u;
  for (int k = tid; k < nc; k += SP_BLOCK) s_cnt[k] = 0;
  __syncthreads();

  unsigned kh[3] = {0u, 0u, 0u}, kl[3] = {0u, 0u, 0u};
  for (int f = tid; f < F; f += SP_BLOCK) {
    SpFace t;
    sp_face(vf, V, faces, f, t);
    if (!t.ok) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) { kh[a] = max(kh[a], float_key(t.hi[a])); kl[a] = max(kl[a], float_key(-t.lo[a])); }
  }
  if (kh[0]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMax(&s_box[a], kh[a]); atomicMax(&s_box[3 + a], kl[a]); }
  }
  __syncthreads();
  float x0[3], sx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float hi = s_box[0] ? float_unkey(s_box[a]) : 0.f, lo = s_box[0] ? -float_unkey(s_box[3 + a]) : 0.f, e = hi - lo;
    x0[a] = lo;
    sx[a] = (e > 0.f && e < GEOM_FMAX) ? (float)G / e : 0.f;
  }

  unsigned kk[3] = {0u, 0u, 0u};
  for (int f = tid; f < F; f += SP_BLOCK) {
    SpFace t;
    sp_face(vf, V, faces, f, t);
    if (!t.ok) continue;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = grid_cell(t.lo[a], x0[a], sx[a], G);
      kk[a] = max(kk[a], (unsigned)(grid_cell(t.hi[a], x0[a], sx[a], G) - c[a]));
    }
    atomicAdd(&s_cnt[(c[2] * G + c[1]) * G + c[0]], 1);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) if (kk[a]) atomicMax(&s_k[a], kk[a]);
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { w.hdr[a] = __float_as_int(x0[a]); w.hdr[3 + a] = __float_as_int(sx[a]); w.hdr[6 + a] = (int)s_k[a]; }
  }
  // exclusive scan of the nc <= 4096 counters; s_cnt becomes the fill cursor
  const int valid = block_exclusive_scan<SP_BLOCK>(nc, s_part, [&](int k) { return s_cnt[k]; }, [&](int k, int acc) { s_cnt[k] = acc; w.cell_start[k] = acc; });
  if (tid == 0) w.cell_start[nc] = valid;                      // the valid faces
  __syncthreads();
  for (int f = tid; f < F; f += SP_BLOCK) {
    SpFace t;
    sp_face(vf, V, faces, f, t);
    if (!t.ok) continue;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = grid_cell(t.lo[a], x0[a], sx[a], G);
    const int slot = atomicAdd(&s_cnt[(c[2] * G + c[1]) * G + c[0]], 1);      // the order inside a cell is free: the fill pass sorts
    w.item[slot] = f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { box[6 * (size_t)slot + a] = t.lo[a]; box[6 * (size_t)slot + 3 + a] = t.hi[a]; }
  }
}

// grid (face block, frame): one face per thread against the faces binned in [cell(min) - K, cell(max)]
template <bool FILL>
__global__ void __launch_bounds__(SP_BLOCK) sp_grid_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F, SpSegm g,
                                                            int G, int* __restrict__ ws, long long wstride, int* __restrict__ pairs, int C) {
  const int b = blockIdx.y, i = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (i >= F) return;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const SpWs<int*> w = sp_ws(ws + (size_t)b * wstride, F, G, LEMO_SELFPEN_GRID);
  int m = 0, base = 0, filled = 0, found = 0;
  if (FILL) {
    m = sp_slice(w.cnt, w.off, i, F, C, base);
    if (m == 0) return;
  }
  int* __restrict__ pr = pairs + ((size_t)b * C + base) * 2;
  const float* __restrict__ box = reinterpret_cast<const float*>(w.box);
  SpFace me;
  sp_face(vf, V, faces, i, me);
  if (me.ok) {
    int lc[3], hc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x0 = __int_as_float(w.hdr[a]), sx = __int_as_float(w.hdr[3 + a]);
      lc[a] = max(grid_cell(me.lo[a], x0, sx, G) - w.hdr[6 + a], 0);
      hc[a] = grid_cell(me.hi[a], x0, sx, G);
    }
    for (int cz = lc[2]; cz <= hc[2]; ++cz)
      for (int cy = lc[1]; cy <= hc[1]; ++cy) {
        const int row = (cz * G + cy) * G;
        const int s0 = w.cell_start[row + lc[0]], s1 = w.cell_start[row + hc[0] + 1];      // the cells of one x-row are contiguous
        for (int s = s0; s < s1; ++s) {
          const int j = w.item[s];
          const float* __restrict__ bj = box + 6 * (size_t)s;
          if (j > i && sp_overlap(me.lo, me.hi, bj[0], bj[1], bj[2], bj[3], bj[4], bj[5])) {
            SpFace other;
            sp_face(vf, V, faces, j, other);
            if (sp_collide(me, other, g, i, j)) {
              if (FILL) sp_insert(pr, m, filled, i, j); else ++found;
            }
          }
        }
      }
  }
  if (!FILL) w.cnt[i] = found;
}

// ---- the cone distance field ---------------------------------------------------------------------------------------------------
// forward-mode dual with N partials; the setup below is written once for float and for SpDual
template <int N> struct SpDual { float v; float d[N]; };
__device__ __forceinline__ float sp_val(float a) { return a; }
template <int N> __device__ __forceinline__ float sp_val(const SpDual<N>& a) { return a.v; }
__device__ __forceinline__ float sp_sqrt(float a) { return sqrtf(a); }
template <int N> __device__ __forceinline__ SpDual<N> sp_sqrt(const SpDual<N>& a) {
  SpDual<N> o;
  o.v = sqrtf(a.v);
  const float s = 0.5f / o.v;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = a.d[k] * s;
  return o;
}
template <int N> __device__ __forceinline__ SpDual<N> operator+(const SpDual<N>& a, const SpDual<N>& b) {
  SpDual<N> o;
  o.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = a.d[k] + b.d[k];
  return o;
}
template <int N> __device__ __forceinline__ SpDual<N> operator-(const SpDual<N>& a, const SpDual<N>& b) {
  SpDual<N> o;
  o.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = a.d[k] - b.d[k];
  return o;
}
template <int N> __device__ __forceinline__ SpDual<N> operator*(const SpDual<N>& a, const SpDual<N>& b) {
  SpDual<N> o;
  o.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return o;
}
template <int N> __device__ __forceinline__ SpDual<N> operator/(const SpDual<N>& a, const SpDual<N>& b) {
  SpDual<N> o;
  const float inv = 1.0f / b.v;
  o.v = a.v * inv;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = (a.d[k] - o.v * b.d[k]) * inv;
  return o;
}
template <int N> __device__ __forceinline__ SpDual<N> operator*(const SpDual<N>& a, float s) {
  SpDual<N> o;
  o.v = a.v * s;
#pragma unroll
  for (int k = 0; k < N; ++k) o.d[k] = a.d[k] * s;
  return o;
}

// triangle (0, q1, q2) -> unit normal n, circumcentre o (relative to p0, barycentric form), circumradius r; false: zero area / not finite
template <typename T> __device__ __forceinline__ bool sp_cone(const T q1[3], const T q2[3], T n[3], T o[3], T& r) {
  const T N0 = q1[1] * q2[2] - q1[2] * q2[1], N1 = q1[2] * q2[0] - q1[0] * q2[2], N2 = q1[0] * q2[1] - q1[1] * q2[0];
  const T A2sq = N0 * N0 + N1 * N1 + N2 * N2;
  if (!(sp_val(A2sq) > 0.f) || !(sp_val(A2sq) < GEOM_FMAX)) return false;
  const T A2 = sp_sqrt(A2sq);
  n[0] = N0 / A2; n[1] = N1 / A2; n[2] = N2 / A2;
  const T d0 = q1[0] - q2[0], d1 = q1[1] - q2[1], d2 = q1[2] - q2[2];
  const T a2 = d0 * d0 + d1 * d1 + d2 * d2;                   // |p1 - p2|^2, opposite p0
  const T b2 = q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2];   // |p2 - p0|^2, opposite p1
  const T c2 = q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2];   // |p0 - p1|^2, opposite p2
  const T w0 = a2 * (b2 + c2 - a2), w1 = b2 * (c2 + a2 - b2), w2 = c2 * (a2 + b2 - c2);
  const T wsum = w0 + w1 + w2;
  if (!(sp_val(wsum) > 0.f) || !(sp_val(wsum) < GEOM_FMAX)) return false;
  const T u1 = w1 / wsum, u2 = w2 / wsum;                      // p0's weight multiplies the origin
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = u1 * q1[k] + u2 * q2[k];
  r = sp_sqrt(a2 * b2 * c2) / (A2 * 2.0f);
  return sp_val(r) > 0.f && sp_val(r) < GEOM_FMAX;
}

// Psi(n, o, r; x) and its partials: d Psi = c_h dh + c_rho drho + c_r dr with dh = n . dd + d . dn, drho = u . dd - h u . dn (u = q / rho,
// 0 at rho == 0), d = x - o.  psi == 0 (outside the cone, or Upsilon == 0): every coefficient is 0.
struct SpPsi { float psi, c_h, c_rho, c_r, h, d[3], u[3]; };

__device__ __forceinline__ void sp_psi(const float n[3], const float o[3], float r, const float x[3], float sigma, int outside, SpPsi& s) {
  s.psi = 0.f; s.c_h = 0.f; s.c_rho = 0.f; s.c_r = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) s.d[k] = x[k] - o[k];
  const float h = n[0] * s.d[0] + n[1] * s.d[1] + n[2] * s.d[2];
  s.h = h;
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = s.d[k] - h * n[k];
  const float rho = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  const float ir = rho > 0.f ? 1.0f / rho : 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) s.u[k] = q[k] * ir;
  const float D = r - (r / sigma) * h;
  if (!(D > 0.f) || !(rho < D)) return;                       // Phi >= 1, a denominator that is not positive, NaN
  float ups, dups;
  if (h <= -sigma) {
    ups = -h + 1.0f - sigma; dups = -1.0f;
  } else if (h < sigma) {
    const float k2 = (1.0f - 2.0f * sigma) / (4.0f * sigma * sigma), k1 = 1.0f / (2.0f * sigma);
    ups = -k2 * h * h - k1 * h + (3.0f - 2.0f * sigma) * 0.25f;
    dups = -2.0f * k2 * h - k1;
  } else {
    return;
  }
  if (!outside && h > 0.f) return;
  const float phi = rho / D;
  s.psi = (1.0f - phi) * ups;
  s.c_h = (1.0f - phi) * dups - ups * phi * (r / sigma) / D;
  s.c_rho = -ups / D;
  s.c_r = ups * phi / r;
}

struct SpTri { int id[3]; float p0[3], q1[3], q2[3]; bool ok; };

// face f of the list -> indices and p0-relative corners; not ok: f or a vertex index out of range
__device__ __forceinline__ void sp_tri(const float* __restrict__ vf, int V, const int* __restrict__ faces, int F, int f, SpTri& t) {
  t.ok = (unsigned)f < (unsigned)F;
  const int ff = t.ok ? f : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) { t.id[k] = faces[3 * (size_t)ff + k]; t.ok = t.ok && (unsigned)t.id[k] < (unsigned)V; }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i0 = t.ok ? t.id[0] : 0, i1 = t.ok ? t.id[1] : 0, i2 = t.ok ? t.id[2] : 0;
    t.p0[k] = vf[3 * (size_t)i0 + k];
    t.q1[k] = vf[3 * (size_t)i1 + k] - t.p0[k];
    t.q2[k] = vf[3 * (size_t)i2 + k] - t.p0[k];
  }
}

// sum over the corners of P of Psi_R(corner)^2
__device__ __forceinline__ float sp_side_fwd(const SpTri& R, const SpTri& P, float sigma, int outside) {
  float n[3], o[3], r;
  if (!sp_cone<float>(R.q1, R.q2, n, o, r)) return 0.f;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (c == 0 ? P.p0[k] : c == 1 ? P.p0[k] + P.q1[k] : P.p0[k] + P.q2[k]) - R.p0[k];
    SpPsi s;
    sp_psi(n, o, r, x, sigma, outside, s);
    acc += s.psi * s.psi;
  }
  return acc;
}

__device__ __forceinline__ int sp_listed(const int* __restrict__ count, int b, int C) { return count ? max(0, min(count[b], C)) : C; }

// one workgroup per frame; a fixed-order sum
__global__ void __launch_bounds__(SP_BLOCK) sp_loss_fwd_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                const int* __restrict__ pairs, int C, const int* __restrict__ count, float sigma,
                                                                int outside, float* __restrict__ loss) {
  __shared__ float s_sum[SP_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const int* __restrict__ pb = pairs + (size_t)b * C * 2;
  const int n = sp_listed(count, b, C);
  float acc = 0.f;
  for (int c = tid; c < n; c += SP_BLOCK) {
    SpTri A, Bt;
    sp_tri(vf, V, faces, F, pb[2 * (size_t)c], A);
    sp_tri(vf, V, faces, F, pb[2 * (size_t)c + 1], Bt);
    if (!A.ok || !Bt.ok) continue;
    acc += sp_side_fwd(A, Bt, sigma, outside) + sp_side_fwd(Bt, A, sigma, outside);
  }
  s_sum[tid] = acc;
  __syncthreads();
  for (int w = SP_BLOCK / 2; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w];
    __syncthreads();
  }
  if (tid == 0) loss[b] = s_sum[0];
}

// where the adjoint of a frame is summed: fp32 atomics on gverts (lemo_selfpen_loss_backward: its bits depend on the order of
// arrival, as they always did) or the 64-bit fixed-point buffer of fixed_acc.hpp (the PROX engine: order-independent)
struct SpAccF32 {
  float* gv;
  __device__ __forceinline__ SpAccF32 frame(size_t off) const { return SpAccF32{gv + off}; }
  __device__ __forceinline__ void add(size_t i, float v) const { atomicAdd(&gv[i], v); }
};
struct SpAccFix {
  long long* gv; int* flag;
  __device__ __forceinline__ SpAccFix frame(size_t off) const { return SpAccFix{gv + LEMO_FIX_WORDS * off, flag}; }
  __device__ __forceinline__ void add(size_t i, float v) const { fix_add(gv, i, v, flag); }
};

// gradient of gl * sum over the corners of P of Psi_R(corner)^2 with respect to the six vertices, added to gv
template <class Acc>
__device__ __forceinline__ void sp_side_bwd(const SpTri& R, const SpTri& P, float sigma, int outside, float gl, const Acc& gv) {
  typedef SpDual<6> D6;
  D6 q1[3], q2[3], n[3], o[3], r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q1[k].v = R.q1[k]; q2[k].v = R.q2[k];
#pragma unroll
    for (int e = 0; e < 6; ++e) { q1[k].d[e] = e == k ? 1.f : 0.f; q2[k].d[e] = e == 3 + k ? 1.f : 0.f; }
  }
  if (!sp_cone<D6>(q1, q2, n, o, r)) return;
  const float nv[3] = {n[0].v, n[1].v, n[2].v}, ov[3] = {o[0].v, o[1].v, o[2].v};
  float Gn[3] = {0.f, 0.f, 0.f}, Go[3] = {0.f, 0.f, 0.f}, Gr = 0.f, Gx[3] = {0.f, 0.f, 0.f};
  bool any = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (c == 0 ? P.p0[k] : c == 1 ? P.p0[k] + P.q1[k] : P.p0[k] + P.q2[k]) - R.p0[k];
    SpPsi s;
    sp_psi(nv, ov, r.v, x, sigma, outside, s);
    const float gp = 2.0f * s.psi * gl;
    if (gp == 0.f || !(fabsf(gp) < GEOM_FMAX)) continue;
    any = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float gd = gp * (s.c_h * nv[k] + s.c_rho * s.u[k]);      // d / dd = d / dx = -d / do
      Gn[k] += gp * (s.c_h * s.d[k] - s.c_rho * s.h * s.u[k]);
      Go[k] -= gd;
      Gx[k] += gd;
      gv.add(3 * (size_t)P.id[c] + k, gd);
    }
    Gr += gp * s.c_r;
  }
  if (!any) return;
  float gq[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    float a = Gr * r.d[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) a += Gn[k] * n[k].d[e] + Go[k] * o[k].d[e];
    gq[e] = a;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gv.add(3 * (size_t)R.id[1] + k, gq[k]);
    gv.add(3 * (size_t)R.id[2] + k, gq[3 + k]);
    gv.add(3 * (size_t)R.id[0] + k, -(gq[k] + gq[3 + k]) - Gx[k]);
  }
}

// grid (pair block, frame); gloss NULL: every frame's loss has the gradient gl_all
template <class Acc>
__global__ void __launch_bounds__(SP_BLOCK) sp_loss_bwd_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                const int* __restrict__ pairs, int C, const int* __restrict__ count, float sigma,
                                                                int outside, const float* __restrict__ gloss, float gl_all, Acc gverts) {
  const int b = blockIdx.y, c = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (c >= sp_listed(count, b, C)) return;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const int* __restrict__ pb = pairs + (size_t)b * C * 2;
  SpTri A, Bt;
  sp_tri(vf, V, faces, F, pb[2 * (size_t)c], A);
  sp_tri(vf, V, faces, F, pb[2 * (size_t)c + 1], Bt);
  if (!A.ok || !Bt.ok) return;
  const float gl = gloss ? gloss[b] : gl_all;
  const Acc gv = gverts.frame((size_t)b * V * 3);
  sp_side_bwd(A, Bt, sigma, outside, gl, gv);
  sp_side_bwd(Bt, A, sigma, outside, gl, gv);
}

namespace {

int sp_shape(int B, int V, int F, int mode, int grid) {
  if (mode < LEMO_SELFPEN_AUTO || mode > LEMO_SELFPEN_GRID) return LEMO_ERR_ARG;
  if (grid < 0 || grid == 1 || grid > SP_GMAX) return LEMO_ERR_ARG;
  if (B < 1 || V < 1 || F < 1 || B > 65535 || F > (1 << 24) || (long long)B * V > (1ll << 30) || (long long)B * F > (1ll << 30)) return LEMO_ERR_SHAPE;
  return 0;
}

int sp_list_shape(int B, int V, int F, int C) {
  if (B < 1 || V < 1 || F < 1 || C < 1 || B > 65535 || F > (1 << 24) || (long long)B * V > (1ll << 30) || (long long)B * C > (1ll << 28)) return LEMO_ERR_SHAPE;
  return 0;
}

long long sp_words(int F, int mode, int G) { return sp_ws(0ll, F, G, mode).end; }

// what `auto` means.  Decided by the run of tools/selfpen_rate.py recorded in profiles/selfpen_rate.txt (MI355X, B = 100, V = 10475,
// F = 20908, arms pushed into the torso): brute force 32.8 ms, grid 16 77.9 ms, grid 8 100.0 ms.  The pushed arms stretch the triangles
// between moved and unmoved vertices over much of the body, K grows to the width of the grid, and every face then visits most cells
// without the LDS streaming of the brute-force kernel.  A pass of their own for such faces (vis_big_kernel's scheme) is the open step.
#define SP_AUTO_MODE LEMO_SELFPEN_BRUTE

}  // namespace

long long selfpen_search_workspace_bytes(int B, int V, int F, int mode, int grid) {
  if (sp_shape(B, V, F, mode, grid)) return -1;
  if (mode == LEMO_SELFPEN_AUTO) mode = SP_AUTO_MODE;
  return 4 * (long long)B * sp_words(F, mode, grid ? grid : SP_GMAX);
}

int selfpen_search(const float* verts, int B, int V, const int* faces, int F, const int* segm, const int* parents, const unsigned char* ign,
                   int P, int mode, int grid, int* pairs, int C, int* count, void* ws, long long ws_bytes, hipStream_t s) {
  if (int e = sp_shape(B, V, F, mode, grid)) return e;
  if (int e = sp_list_shape(B, V, F, C)) return e;
  if (!verts || !faces || !pairs || !count || !ws || P < 0 || P > SP_PMAX || (ign && P < 1) || (!ign && P != 0) || ((parents || ign) && !segm))
    return LEMO_ERR_ARG;
  if (mode == LEMO_SELFPEN_AUTO) mode = SP_AUTO_MODE;
  const int G = grid ? grid : SP_GMAX;
  const long long words = sp_words(F, mode, G);
  if (ws_bytes < 4 * (long long)B * words) return LEMO_ERR_ARG;
  int* w = static_cast<int*>(ws);
  const SpSegm g = {segm, parents, ign, P};
  const dim3 blk(SP_BLOCK), gf((F + SP_BLOCK - 1) / SP_BLOCK, B);
  if (mode == LEMO_SELFPEN_BRUTE) {
    hipLaunchKernelGGL(sp_brute_kernel<false>, gf, blk, 0, s, verts, V, faces, F, g, w, words, pairs, C);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(B), blk, 0, s, F, w, words, pairs, C, count);
    hipLaunchKernelGGL(sp_brute_kernel<true>, gf, blk, 0, s, verts, V, faces, F, g, w, words, pairs, C);
  } else {
    hipLaunchKernelGGL(sp_bin_kernel, dim3(B), blk, 0, s, verts, V, faces, F, G, w, words);
    hipLaunchKernelGGL(sp_grid_kernel<false>, gf, blk, 0, s, verts, V, faces, F, g, G, w, words, pairs, C);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(B), blk, 0, s, F, w, words, pairs, C, count);
    hipLaunchKernelGGL(sp_grid_kernel<true>, gf, blk, 0, s, verts, V, faces, F, g, G, w, words, pairs, C);
  }
  return (int)hipGetLastError();
}

static int sp_loss_args(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, float sigma) {
  if (int e = sp_list_shape(B, V, F, C)) return e;
  if (!verts || !faces || !pairs || !(sigma > 0.f) || !std::isfinite(sigma)) return LEMO_ERR_ARG;
  return 0;
}

int selfpen_loss_forward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                         int penalize_outside, float* loss, hipStream_t s) {
  if (int e = sp_loss_args(verts, B, V, faces, F, pairs, C, sigma)) return e;
  if (!loss) return LEMO_ERR_ARG;
  hipLaunchKernelGGL(sp_loss_fwd_kernel, dim3(B), dim3(SP_BLOCK), 0, s, verts, V, faces, F, pairs, C, count, sigma, penalize_outside ? 1 : 0, loss);
  return (int)hipGetLastError();
}

int selfpen_loss_backward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                          int penalize_outside, const float* gloss, float* gverts, hipStream_t s) {
  if (int e = sp_loss_args(verts, B, V, faces, F, pairs, C, sigma)) return e;
  if (!gloss || !gverts) return LEMO_ERR_ARG;
  if (hipError_t e = hipMemsetAsync(gverts, 0, (size_t)B * V * 3 * sizeof(float), s)) return (int)e;
  hipLaunchKernelGGL(sp_loss_bwd_kernel<SpAccF32>, dim3((C + SP_BLOCK - 1) / SP_BLOCK, B), dim3(SP_BLOCK), 0, s, verts, V, faces, F, pairs, C, count,
                     sigma, penalize_outside ? 1 : 0, gloss, 0.f, SpAccF32{gverts});
  return (int)hipGetLastError();
}

// the PROX engine's form: gl * dL[b] / dverts of every frame ADDED to the fixed-point buffer acc [B][V][3] (fixed_acc.hpp; the caller
// zeroes and converts it; two words per entry), so that the sum does not depend on the order of arrival
int selfpen_loss_backward_fixed(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                                int penalize_outside, float gl, long long* acc, int* flag, hipStream_t s) {
  if (int e = sp_loss_args(verts, B, V, faces, F, pairs, C, sigma)) return e;
  if (!acc || !flag) return LEMO_ERR_ARG;
  hipLaunchKernelGGL(sp_loss_bwd_kernel<SpAccFix>, dim3((C + SP_BLOCK - 1) / SP_BLOCK, B), dim3(SP_BLOCK), 0, s, verts, V, faces, F, pairs, C, count,
                     sigma, penalize_outside ? 1 : 0, (const float*)nullptr, gl, SpAccFix{acc, flag});
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
long long lemo_selfpen_search_workspace_bytes(int B, int V, int F, int mode, int grid) {
  return lemo::selfpen_search_workspace_bytes(B, V, F, mode, grid);
}
int lemo_selfpen_search(const float* verts, int B, int V, const int* faces, int F, const int* segm, const int* parents, const unsigned char* ign,
                        int P, int mode, int grid, int* pairs, int C, int* count, void* ws, long long ws_bytes, void* stream) {
  return lemo::selfpen_search(verts, B, V, faces, F, segm, parents, ign, P, mode, grid, pairs, C, count, ws, ws_bytes, (hipStream_t)stream);
}
int lemo_selfpen_loss_forward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                              int penalize_outside, float* loss, void* stream) {
  return lemo::selfpen_loss_forward(verts, B, V, faces, F, pairs, C, count, sigma, penalize_outside, loss, (hipStream_t)stream);
}
int lemo_selfpen_loss_backward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                               int penalize_outside, const float* gloss, float* gverts, void* stream) {
  return lemo::selfpen_loss_backward(verts, B, V, faces, F, pairs, C, count, sigma, penalize_outside, gloss, gverts, (hipStream_t)stream);
}
}  // extern "C"
