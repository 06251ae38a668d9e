// The signed-distance volume of a scene mesh: what the PROX fit reads through sdf_at (scene_device.hpp) at every vertex of every frame
// (fitting_temp_slide.py:685-739).  The reference loads it from <scene>.json and <scene>_sdf.npy (fit_temp_loadprox_slide.py:286-299);
// the program that made those files was never published, so the definition below is this project's, NOT a restatement of it.
//
// Volume.  sdf[ix][iy][iz], fp32, D x H x W = x, y, z.  The centre of voxel i on axis a is gmin[a] + (i + 0.5) (gmax[a] - gmin[a]) / dim[a]
// (here: fmaf(i + 0.5, step[a], gmin[a]) with step = (gmax - gmin) / dim formed in fp32 on the host) -- the point where sdf_at has
// interpolation weight 0, so sampling the built volume at its own centres gives the volume back.  Whether PROX's generator sampled at
// these centres is unknown.
// Magnitude.  The exact Euclidean distance from the centre to the nearest point of the triangle soup: closest point on a triangle by
// Voronoi region (Ericson, Real-Time Collision Detection 5.1.5; all seven regions), every valid triangle of the mesh is a candidate, no
// truncation band, no sweep.  A triangle is IGNORED iff a vertex index lies outside [0, V), a coordinate is not finite, or its row of
// the face-normal table is zero (the host marks zero-area triangles that way: one rule, decided once per mesh, the same in every
// mode).  No valid triangle: +inf everywhere, nearest = -1.
// Sign.  Negative where (p - c) . n < 0, c the closest point and n the angle-weighted pseudonormal (Baerentzen & Aanaes 2005) of the
// feature c lies on: the face normal inside a face, edge_n[f][e] on edge e (0: v0 v1, 1: v1 v2, 2: v2 v0; the sum of the unit normals
// of the faces sharing that undirected edge), vert_n[v] at a vertex (unit normals of the incident faces weighted by their corner
// angles).  (p - c) . n == 0 counts as positive.  Closed outward-oriented mesh: inside / outside.  PROX's single-sided scans: "behind
// the surface", which is what makes a foot under the floor negative.  The tables depend on the mesh alone; the host builds them once in
// float64 and rounds to fp32.  Only the winner's rows are read, once per voxel: the inner loop is distance only.
// Winner.  The smallest squared distance, then the lowest face index.  sdf_closest(p; a, ab, ac) is ONE device function, fp32 VALU with
// explicit fmaf and contraction off, fed the same (a, b - a, c - a) in every mode: the result cannot depend on who enumerates the
// candidates.
//
// BRUTE (the yardstick mode): chamfer_nn_kernel's structure.  A workgroup owns a brick of 4 x 8 x 8 voxels, one per thread, in
// registers; every triangle is streamed through LDS in chunks of 256 as ten arrays (a, b - a, c - a, face index) read at a wave-uniform
// address (a broadcast), two buffers, one barrier per chunk, 20 KB of static LDS.
// GRID (the product mode): a G^3 cell grid over the volume's box.
//   sdf_count / sdf_scan / sdf_fill : counting sort.  A valid triangle whose box (clamped to the volume's box: clamping is the projection
//                 onto a convex set that holds every voxel, so it never lengthens a distance to a voxel) touches at most two cells per
//                 axis is SMALL and goes to the cell of its min corner; every other one is BIG and goes to a list that each brick
//                 scans whole.  (a, b - a, c - a, index) is stored in cell order.  Slots come from integer fetch-adds: the order inside
//                 a cell is free, and the winner rule makes the output independent of it.
//   sdf_cheb    : per cell, the Chebyshev distance to the nearest cell that holds a small triangle (three separable passes).
//   sdf_grid    : the brick's voxels lie in the cell range [bl, bh].  Shell r = the cells at Chebyshev distance r from that range.  The
//                 first shell that holds anything is min cheb over the range: empty space is skipped in one step.  From there shells
//                 are visited outward.  A row segment of a shell (cells x0 .. x1 of one (y, z): contiguous in the sorted order) holds
//                 triangles inside [cell_lo(x0), cell_lo(x1) + 2 h] x ..., and is skipped iff the distance from the brick's box to that
//                 box, shrunk by the slack below, exceeds the largest best-so-far of the brick.  Everything in shell r or beyond is at
//                 least (r - 2) min(h) away; the search ends when that, shrunk, exceeds the brick's largest best-so-far.
//   Slack.  A computed d^2 differs from the true one by roundings of a few ulp of the largest coordinate M (mesh and box) in p - c, and
//   the cell of a coordinate by one rounding of M.  A bound L is used as L (1 - 2^-12) - 2^-14 M, squared, and compared with `>`:
//   16 times the error estimate (about 50 ulp of M = 2^-18 M), so a triangle that could win, or tie and win on its index, is never
//   skipped.  GRID therefore equals BRUTE bit for bit, the nearest-face volume included, for every G.
// AUTO: see SDF_AUTO_FACES below.  No allocation (caller's workspace), no host synchronisation, capturable in a graph.
#include "geom_device.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace lemo {

#define SDF_BLOCK 256
#define SDF_CHUNK 256                                        // triangles per LDS buffer
#define SDF_BX 4                                             // brick: 4 x 8 x 8 voxels (x, y, z), z fastest over the threads
#define SDF_BY 8
#define SDF_BZ 8
#define SDF_GMAX 32                                          // largest grid side
#define SDF_HDR 16                                           // words of the workspace header: [0] big triangles, [1] bits of max |coordinate|
#define SDF_TW 10                                            // words of a stored triangle
#define SDF_TASKS 128                                        // shell rows examined per round: at most two segments each
#define SDF_CHEB_INF (1 << 20)

struct SdfGeom { float g0[3], step[3]; int dim[3]; };
struct SdfMesh { const float* verts; int V; const int* faces; int F; const float* face_n; };

// Ericson's closest point by Voronoi region, for p against the triangle (a, a + ab, a + ac) -> d^2; q = p - c;
// feat: 0 face, 1 .. 3 edge v0 v1 / v1 v2 / v2 v0, 4 .. 6 vertex v0 / v1 / v2.  The regions are tested in Ericson's order (the
// overrides below run backwards, so the first that holds wins).  One division.
__device__ __forceinline__ float sdf_closest(const float p[3], const float a[3], const float ab[3], const float ac[3], float q[3], int& feat) {
  float ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ap[k] = p[k] - a[k]; bp[k] = ap[k] - ab[k]; cp[k] = ap[k] - ac[k]; }
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = fmaf(d1, d4, -(d3 * d2)), vb = fmaf(d5, d2, -(d1 * d6)), va = fmaf(d3, d6, -(d5 * d4));
  const float e43 = d4 - d3, e56 = d5 - d6;
  float ns = vb, nt = vc, dn = va + vb + vc;
  int ft = 0;
  if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { ns = e56; nt = e43; dn = e43 + e56; ft = 2; }
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { ns = 0.f; nt = d2; dn = d2 - d6; ft = 3; }
  if (d6 >= 0.f && d5 <= d6) { ns = 0.f; nt = 1.f; dn = 1.f; ft = 6; }
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { ns = d1; nt = 0.f; dn = d1 - d3; ft = 1; }
  if (d3 >= 0.f && d4 <= d3) { ns = 1.f; nt = 0.f; dn = 1.f; ft = 5; }
  if (d1 <= 0.f && d2 <= 0.f) { ns = 0.f; nt = 0.f; dn = 1.f; ft = 4; }
  const float inv = 1.0f / dn, s = ns * inv, t = nt * inv;
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = fmaf(-t, ac[k], fmaf(-s, ab[k], ap[k]));
  feat = ft;
  return dot3(q, q);
}

// face f -> the ten stored words (a, b - a, c - a, index); false: ignored (out[9] = -1)
__device__ __forceinline__ bool sdf_tri_load(const SdfMesh& m, int f, float out[SDF_TW], float lo[3], float hi[3]) {
  int id[3];
  float c[3][3];
  const bool ids = face_ids(m.faces, f, m.V, id);
  bool ok = face_corners(m.verts, id, ids, c);
  const float n0 = m.face_n[3 * (size_t)f], n1 = m.face_n[3 * (size_t)f + 1], n2 = m.face_n[3 * (size_t)f + 2];
  ok = ok && (n0 != 0.f || n1 != 0.f || n2 != 0.f);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out[a] = c[0][a]; out[3 + a] = c[1][a] - c[0][a]; out[6 + a] = c[2][a] - c[0][a];
    lo[a] = fminf(c[0][a], fminf(c[1][a], c[2][a]));
    hi[a] = fmaxf(c[0][a], fmaxf(c[1][a], c[2][a]));
  }
  out[9] = __int_as_float(ok ? f : -1);
  return ok;
}

// the thread's voxel of brick `blk`; false: outside the volume (the thread still takes part in every barrier)
__device__ __forceinline__ bool sdf_voxel(const SdfGeom& g, int blk, int tid, int ix[3], float p[3], int b0[3]) {
  const int nby = (g.dim[1] + SDF_BY - 1) / SDF_BY, nbz = (g.dim[2] + SDF_BZ - 1) / SDF_BZ;
  b0[2] = (blk % nbz) * SDF_BZ; b0[1] = ((blk / nbz) % nby) * SDF_BY; b0[0] = (blk / (nbz * nby)) * SDF_BX;
  ix[2] = b0[2] + (tid & 7); ix[1] = b0[1] + ((tid >> 3) & 7); ix[0] = b0[0] + (tid >> 6);
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    in = in && ix[a] < g.dim[a];
    p[a] = fmaf((float)min(ix[a], g.dim[a] - 1) + 0.5f, g.step[a], g.g0[a]);
  }
  return in;
}

// the candidates of one LDS buffer against the thread's voxel
__device__ __forceinline__ void sdf_scan_buffer(const float (*sb)[SDF_CHUNK], int n, const float p[3], float& best, int& bf) {
  for (int jj = 0; jj < n; ++jj) {
    const int id = __float_as_int(sb[9][jj]);
    if (id < 0) continue;                                     // wave-uniform
    const float a[3] = {sb[0][jj], sb[1][jj], sb[2][jj]}, ab[3] = {sb[3][jj], sb[4][jj], sb[5][jj]}, ac[3] = {sb[6][jj], sb[7][jj], sb[8][jj]};
    float q[3];
    int ft;
    const float d2 = sdf_closest(p, a, ab, ac, q, ft);
    if (d2 < best || (d2 == best && id < bf)) { best = d2; bf = id; }
  }
}

// `total` candidates, candidate k produced by fetch(k, stage), against the thread's voxel: two buffers, one barrier per chunk.
// Every thread of the workgroup calls it with the same total.
template <typename Fetch>
__device__ __forceinline__ void sdf_stream(float (*sb)[SDF_TW][SDF_CHUNK], int total, Fetch fetch, const float p[3], float& best, int& bf) {
  if (total <= 0) return;
  const int tid = threadIdx.x;
  float stage[SDF_TW];
  auto get = [&](int c0) {
    if (c0 + tid < total) fetch(c0 + tid, stage);
    else stage[9] = __int_as_float(-1);
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int w = 0; w < SDF_TW; ++w) sb[buf][w][tid] = stage[w];
  };
  get(0);
  __syncthreads();                                            // the previous user of buffer 0 is done
  put(0);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < total; c0 += SDF_CHUNK, buf ^= 1) {
    const bool more = c0 + SDF_CHUNK < total;
    if (more) get(c0 + SDF_CHUNK);
    sdf_scan_buffer(sb[buf], min(SDF_CHUNK, total - c0), p, best, bf);
    if (more) put(buf ^ 1);
    __syncthreads();
  }
}

// the winner -> signed distance and nearest face
__device__ __forceinline__ void sdf_finish(const SdfMesh& m, const float* __restrict__ edge_n, const float* __restrict__ vert_n, const SdfGeom& g,
                                           const int ix[3], const float p[3], float best, int bf, float* __restrict__ sdf, int* __restrict__ nearest) {
  const size_t o = ((size_t)ix[0] * g.dim[1] + ix[1]) * g.dim[2] + ix[2];
  float val = INFINITY;
  if (bf >= 0) {
    float t[SDF_TW], lo[3], hi[3], q[3];
    int ft;
    sdf_tri_load(m, bf, t, lo, hi);
    const float a[3] = {t[0], t[1], t[2]}, ab[3] = {t[3], t[4], t[5]}, ac[3] = {t[6], t[7], t[8]};
    const float d2 = sdf_closest(p, a, ab, ac, q, ft);      // the same bits as in the search
    const float* __restrict__ np = ft == 0 ? m.face_n + 3 * (size_t)bf
                                  : ft <= 3 ? edge_n + 9 * (size_t)bf + 3 * (ft - 1)
                                            : vert_n + 3 * (size_t)m.faces[3 * (size_t)bf + (ft - 4)];
    const float n[3] = {np[0], np[1], np[2]};
    const float d = sqrtf(d2);
    val = dot3(q, n) < 0.f ? -d : d;
  }
  sdf[o] = val;
  if (nearest) nearest[o] = bf;
}

// ---- brute force ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SDF_BLOCK) sdf_brute_kernel(SdfMesh m, const float* __restrict__ edge_n, const float* __restrict__ vert_n, SdfGeom g,
                                                               float* __restrict__ sdf, int* __restrict__ nearest) {
  __shared__ __attribute__((aligned(16))) float sb[2][SDF_TW][SDF_CHUNK];
  int ix[3], b0[3];
  float p[3];
  const bool in = sdf_voxel(g, blockIdx.x, threadIdx.x, ix, p, b0);
  float best = INFINITY;
  int bf = -1;
  sdf_stream(sb, m.F, [&](int k, float* stage) { float lo[3], hi[3]; sdf_tri_load(m, k, stage, lo, hi); }, p, best, bf);
  if (in) sdf_finish(m, edge_n, vert_n, g, ix, p, best, bf, sdf, nearest);
}

// ---- grid ------------------------------------------------------------------------------------------------------------------------
struct SdfGrid { int G; float x0[3], sx[3], h[3]; };      // sx = G / extent, h = extent / G

// workspace words: hdr [SDF_HDR], cnt [nc], cell_start [nc + 1], cursor [nc], cheb_a [nc], cheb_b [nc], tri [F][SDF_TW]
struct SdfWs { int* hdr; int* cnt; int* cell_start; int* cursor; int* cheb_a; int* cheb_b; float* tri; };
static inline SdfWs sdf_ws(void* ws, int G) {
  const size_t nc = (size_t)G * G * G;
  SdfWs w;
  w.hdr = static_cast<int*>(ws); w.cnt = w.hdr + SDF_HDR; w.cell_start = w.cnt + nc; w.cursor = w.cell_start + nc + 1;
  w.cheb_a = w.cursor + nc; w.cheb_b = w.cheb_a + nc; w.tri = reinterpret_cast<float*>(w.cheb_b + nc);
  return w;
}

// -> cell index of a small triangle, -1 for a big one
__device__ __forceinline__ int sdf_tri_cell(const SdfGrid& gr, const float lo[3], const float hi[3]) {
  int c[3];
  bool small = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = grid_cell(lo[a], gr.x0[a], gr.sx[a], gr.G);
    small = small && grid_cell(hi[a], gr.x0[a], gr.sx[a], gr.G) - c[a] <= 1;
  }
  return small ? (c[2] * gr.G + c[1]) * gr.G + c[0] : -1;
}

template <bool FILL>
__global__ void __launch_bounds__(SDF_BLOCK) sdf_bin_kernel(SdfMesh m, SdfGrid gr, SdfWs w) {
  const int f = blockIdx.x * SDF_BLOCK + threadIdx.x;
  if (f >= m.F) return;
  float t[SDF_TW], lo[3], hi[3];
  if (!sdf_tri_load(m, f, t, lo, hi)) return;
  const int c = sdf_tri_cell(gr, lo, hi);
  if (!FILL) {
    if (c >= 0) __hip_atomic_fetch_add(&w.cnt[c], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float mx = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) mx = fmaxf(mx, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    atomicMax(reinterpret_cast<unsigned*>(&w.hdr[1]), __float_as_uint(mx));      // bit patterns of non-negative floats are ordered
    return;
  }
  // small: the cell's next slot; big: from the end of the array downwards.  The order is free: the winner rule does not see it.
  const int slot = c >= 0 ? __hip_atomic_fetch_add(&w.cursor[c], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                          : m.F - 1 - __hip_atomic_fetch_add(&w.hdr[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < SDF_TW; ++k) w.tri[SDF_TW * (size_t)slot + k] = t[k];
}

// exclusive scan of the nc <= 32768 counters (one workgroup): cell_start, and the fill cursors
__global__ void __launch_bounds__(SDF_BLOCK) sdf_scan_kernel(int nc, SdfWs w) {
  __shared__ int s_part[SDF_BLOCK];
  const int total = block_exclusive_scan<SDF_BLOCK>(nc, s_part, [&](int k) { return w.cnt[k]; }, [&](int k, int acc) { w.cell_start[k] = acc; w.cursor[k] = acc; });
  if (threadIdx.x == 0) w.cell_start[nc] = total;
}

// one separable pass of the Chebyshev distance transform along AXIS: out(c) = min over o on the line of max(|c - o|, in(o));
// pass 0 reads the occupancy (in = 0 where the cell holds a triangle, else infinite)
template <int AXIS>
__global__ void __launch_bounds__(SDF_BLOCK) sdf_cheb_kernel(int G, const int* __restrict__ cell_start, const int* __restrict__ in, int* __restrict__ out) {
  const int c = blockIdx.x * SDF_BLOCK + threadIdx.x;
  if (c >= G * G * G) return;
  const int stride = AXIS == 0 ? 1 : AXIS == 1 ? G : G * G;
  const int me = (c / stride) % G, base = c - me * stride;
  int best = SDF_CHEB_INF;
  for (int o = 0; o < G; ++o) {
    const int k = base + o * stride;
    const int v = AXIS == 0 ? (cell_start[k + 1] > cell_start[k] ? 0 : SDF_CHEB_INF) : in[k];
    best = min(best, max(abs(me - o), v));
  }
  out[c] = best;
}

// squared distance between the boxes [alo, ahi] and [blo, bhi], each gap shrunk by the slack (see the header); 0 where they may touch
__device__ __forceinline__ float sdf_box_gap2(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3], float slack) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gap = fmaxf(blo[a] - ahi[a], alo[a] - bhi[a]);
    const float ge = fmaxf(gap * (1.0f - 0x1p-12f) - slack, 0.f);
    s = fmaf(ge, ge, s);
  }
  return s * (1.0f - 0x1p-12f);
}

__global__ void __launch_bounds__(SDF_BLOCK) sdf_grid_kernel(SdfMesh m, const float* __restrict__ edge_n, const float* __restrict__ vert_n, SdfGeom g,
                                                              SdfGrid gr, SdfWs w, float* __restrict__ sdf, int* __restrict__ nearest) {
  __shared__ __attribute__((aligned(16))) float sb[2][SDF_TW][SDF_CHUNK];
  __shared__ int s_start[2 * SDF_TASKS], s_pre[2 * SDF_TASKS + 1];
  __shared__ int s_nseg;
  __shared__ unsigned s_bmax;
  const int tid = threadIdx.x, G = gr.G;
  int ix[3], b0[3];
  float p[3];
  const bool in = sdf_voxel(g, blockIdx.x, tid, ix, p, b0);
  float best = INFINITY;
  int bf = -1;

  // the brick: its box and its cell range (wave-uniform)
  float blo[3], bhi[3];
  int bl[3], bh[3];
  const int bdim[3] = {SDF_BX, SDF_BY, SDF_BZ};
  float M = __uint_as_float((unsigned)w.hdr[1]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    blo[a] = fmaf((float)b0[a] + 0.5f, g.step[a], g.g0[a]);
    bhi[a] = fmaf((float)min(b0[a] + bdim[a], g.dim[a]) - 0.5f, g.step[a], g.g0[a]);
    bl[a] = grid_cell(fminf(blo[a], bhi[a]), gr.x0[a], gr.sx[a], G);
    bh[a] = grid_cell(fmaxf(blo[a], bhi[a]), gr.x0[a], gr.sx[a], G);
    M = fmaxf(M, fmaxf(fabsf(gr.x0[a]), fabsf(gr.x0[a] + gr.h[a] * (float)G)));
  }
  const float slack = M * 0x1p-14f;
  const float hmin = fminf(gr.h[0], fminf(gr.h[1], gr.h[2]));

  // the big triangles, whole
  const int nbig = w.hdr[0];
  {
    const float* __restrict__ big = w.tri + SDF_TW * (size_t)(m.F - nbig);
    sdf_stream(sb, nbig, [&](int k, float* stage) {
#pragma unroll
      for (int q = 0; q < SDF_TW; ++q) stage[q] = big[SDF_TW * (size_t)k + q];
    }, p, best, bf);
  }

  // the first shell that holds anything, and the last that lies inside the grid
  int r = SDF_CHEB_INF, rmax = 0;
  for (int cz = bl[2]; cz <= bh[2]; ++cz)
    for (int cy = bl[1]; cy <= bh[1]; ++cy)
      for (int cx = bl[0]; cx <= bh[0]; ++cx) r = min(r, w.cheb_a[(cz * G + cy) * G + cx]);
#pragma unroll
  for (int a = 0; a < 3; ++a) rmax = max(rmax, max(bl[a], G - 1 - bh[a]));

  for (; r <= rmax; ++r) {
    // the brick's largest best-so-far (invalid threads carry copies of valid voxels: sdf_voxel clamps)
    __syncthreads();
    if (tid == 0) s_bmax = 0u;
    __syncthreads();
    atomicMax(&s_bmax, __float_as_uint(best));                // best >= 0 or +inf: ordered as unsigned
    __syncthreads();
    const float bmax = __uint_as_float(s_bmax);
    {
      const float L = (float)max(r - 2, 0) * hmin, Le = fmaxf(L * (1.0f - 0x1p-12f) - slack, 0.f);
      if (Le * Le * (1.0f - 0x1p-12f) > bmax) break;          // uniform
    }
    const int y0 = bl[1] - r, z0 = bl[2] - r, ny = bh[1] - bl[1] + 1 + 2 * r, nz = bh[2] - bl[2] + 1 + 2 * r;
    const int xa = bl[0] - r, xb = bh[0] + r;
    for (int t0 = 0; t0 < ny * nz; t0 += SDF_TASKS) {
      __syncthreads();
      if (tid == 0) s_nseg = 0;
      __syncthreads();
      const int t = t0 + tid;
      if (tid < SDF_TASKS && t < ny * nz) {
        const int cy = y0 + t % ny, cz = z0 + t / ny;
        if (cy >= 0 && cy < G && cz >= 0 && cz < G) {
          const bool rim = r == 0 || cy == y0 || cy == y0 + ny - 1 || cz == z0 || cz == z0 + nz - 1;
          const int row = (cz * G + cy) * G;
          // rim rows: the whole segment; inner rows: the two end cells
          for (int e = 0; e < (rim ? 1 : 2); ++e) {
            int x0 = rim ? max(xa, 0) : (e == 0 ? xa : xb), x1 = rim ? min(xb, G - 1) : x0;
            if (x0 < 0 || x1 >= G) continue;
            const int s0 = w.cell_start[row + x0], s1 = w.cell_start[row + x1 + 1];
            if (s1 <= s0) continue;
            const float clo[3] = {fmaf((float)x0, gr.h[0], gr.x0[0]), fmaf((float)cy, gr.h[1], gr.x0[1]), fmaf((float)cz, gr.h[2], gr.x0[2])};
            const float chi[3] = {fmaf((float)(x1 + 2), gr.h[0], gr.x0[0]), fmaf((float)(cy + 2), gr.h[1], gr.x0[1]), fmaf((float)(cz + 2), gr.h[2], gr.x0[2])};
            if (sdf_box_gap2(blo, bhi, clo, chi, slack) > bmax) continue;
            const int slot = atomicAdd(&s_nseg, 1);           // LDS; the order is free
            s_start[slot] = s0;
            s_pre[slot + 1] = s1 - s0;
          }
        }
      }
      __syncthreads();
      const int nseg = s_nseg;
      if (tid == 0) {
        int acc = 0;
        s_pre[0] = 0;
        for (int k = 0; k < nseg; ++k) { acc += s_pre[k + 1]; s_pre[k + 1] = acc; }
      }
      __syncthreads();
      const int total = s_pre[nseg];
      sdf_stream(sb, total, [&](int k, float* stage) {
        int a = 0, b = nseg - 1;                              // the segment with s_pre[a] <= k < s_pre[a + 1]
        while (a < b) { const int mid = (a + b + 1) >> 1; if (s_pre[mid] <= k) a = mid; else b = mid - 1; }
        const float* __restrict__ src = w.tri + SDF_TW * (size_t)(s_start[a] + (k - s_pre[a]));
#pragma unroll
        for (int q = 0; q < SDF_TW; ++q) stage[q] = src[q];
      }, p, best, bf);
    }
  }
  if (in) sdf_finish(m, edge_n, vert_n, g, ix, p, best, bf, sdf, nearest);
}

namespace {

// what `auto` means: GRID for F >= SDF_AUTO_FACES, else BRUTE.  Decided by the run of tools/scene_sdf_rate.py recorded in
// profiles/scene_sdf_rate.txt (MI355X, 128^3, a box whose faces are cut into F triangles; median ms, brute force / grid):
// F = 12: 0.090 / 0.124, 48: 0.222 / 0.256, 104: 0.415 / 0.444, 188: 0.682 / 0.698, 428: 1.460 / 1.407, 752: 2.51 / 1.35,
// 3036: 9.9 / 2.0, 12144: 39.9 / 7.6.  The grid build is seven small launches and a shell walk per brick whatever the mesh; brute
// force is F distance evaluations per voxel.  The two cross between 188 and 428 faces.
#define SDF_AUTO_FACES 256

int sdf_default_grid(int D, int H, int W) {
  const int side = std::max(D, std::max(H, W));
  return std::min(SDF_GMAX, std::max(2, side / 8));
}

int sdf_shape(int F, int D, int H, int W, int mode, int grid) {
  if (mode < LEMO_SCENE_SDF_AUTO || mode > LEMO_SCENE_SDF_GRID) return LEMO_ERR_ARG;
  if (grid < 0 || grid == 1 || grid > SDF_GMAX) return LEMO_ERR_ARG;
  if (F < 1 || D < 1 || H < 1 || W < 1 || F > (1 << 22) || D > 1024 || H > 1024 || W > 1024 || (long long)D * H * W > (1ll << 28)) return LEMO_ERR_SHAPE;
  return 0;
}

int sdf_mode(int F, int mode) { return mode == LEMO_SCENE_SDF_AUTO ? (F >= SDF_AUTO_FACES ? LEMO_SCENE_SDF_GRID : LEMO_SCENE_SDF_BRUTE) : mode; }

long long sdf_words(int F, int G) { const long long nc = (long long)G * G * G; return SDF_HDR + 5 * nc + 1 + (long long)SDF_TW * F; }

}  // namespace

long long scene_sdf_ws_bytes(int F, int D, int H, int W, int mode, int grid) {
  if (sdf_shape(F, D, H, W, mode, grid)) return -1;
  if (sdf_mode(F, mode) == LEMO_SCENE_SDF_BRUTE) return 0;
  return 4 * sdf_words(F, grid ? grid : sdf_default_grid(D, H, W));
}

int scene_sdf_build(const float* verts, int V, const int* faces, int F, const float* face_n, const float* edge_n, const float* vert_n,
                    const float* gmin, const float* gmax, int D, int H, int W, int mode, int grid, float* sdf, int* nearest, void* ws,
                    long long ws_bytes, hipStream_t s) {
  if (int e = sdf_shape(F, D, H, W, mode, grid)) return e;
  if (V < 1 || V > (1 << 24)) return LEMO_ERR_SHAPE;
  if (!verts || !faces || !face_n || !edge_n || !vert_n || !gmin || !gmax || !sdf) return LEMO_ERR_ARG;
  SdfGeom g;
  SdfGrid gr;
  mode = sdf_mode(F, mode);
  const int G = grid ? grid : sdf_default_grid(D, H, W);
  const int dim[3] = {D, H, W};
  for (int a = 0; a < 3; ++a) {
    const float e = gmax[a] - gmin[a];
    if (!std::isfinite(gmin[a]) || !std::isfinite(gmax[a]) || !(e > 0.f) || !std::isfinite(e)) return LEMO_ERR_ARG;
    g.g0[a] = gmin[a]; g.step[a] = e / (float)dim[a]; g.dim[a] = dim[a];
    gr.x0[a] = gmin[a]; gr.sx[a] = (float)G / e; gr.h[a] = e / (float)G;
    if (!(g.step[a] > 0.f) || !std::isfinite(gr.sx[a]) || !(gr.h[a] > 0.f)) return LEMO_ERR_ARG;
  }
  gr.G = G;
  const SdfMesh m = {verts, V, faces, F, face_n};
  const int nbrick = ((D + SDF_BX - 1) / SDF_BX) * ((H + SDF_BY - 1) / SDF_BY) * ((W + SDF_BZ - 1) / SDF_BZ);
  const dim3 blk(SDF_BLOCK);
  if (mode == LEMO_SCENE_SDF_BRUTE) {
    hipLaunchKernelGGL(sdf_brute_kernel, dim3(nbrick), blk, 0, s, m, edge_n, vert_n, g, sdf, nearest);
    return (int)hipGetLastError();
  }
  if (!ws || ws_bytes < 4 * sdf_words(F, G)) return LEMO_ERR_ARG;
  const int nc = G * G * G;
  const SdfWs w = sdf_ws(ws, G);
  if (hipError_t e = hipMemsetAsync(w.hdr, 0, sizeof(int) * ((size_t)SDF_HDR + nc), s)) return (int)e;
  const dim3 gf((F + SDF_BLOCK - 1) / SDF_BLOCK), gc((nc + SDF_BLOCK - 1) / SDF_BLOCK);
  hipLaunchKernelGGL(sdf_bin_kernel<false>, gf, blk, 0, s, m, gr, w);
  hipLaunchKernelGGL(sdf_scan_kernel, dim3(1), blk, 0, s, nc, w);
  hipLaunchKernelGGL(sdf_bin_kernel<true>, gf, blk, 0, s, m, gr, w);
  hipLaunchKernelGGL(sdf_cheb_kernel<0>, gc, blk, 0, s, G, w.cell_start, w.cheb_b, w.cheb_a);
  hipLaunchKernelGGL(sdf_cheb_kernel<1>, gc, blk, 0, s, G, w.cell_start, w.cheb_a, w.cheb_b);
  hipLaunchKernelGGL(sdf_cheb_kernel<2>, gc, blk, 0, s, G, w.cell_start, w.cheb_b, w.cheb_a);
  hipLaunchKernelGGL(sdf_grid_kernel, dim3(nbrick), blk, 0, s, m, edge_n, vert_n, g, gr, w, sdf, nearest);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
long long lemo_scene_sdf_ws_bytes(int F, int D, int H, int W, int mode, int grid) { return lemo::scene_sdf_ws_bytes(F, D, H, W, mode, grid); }
int lemo_scene_sdf_build(const float* verts, int V, const int* faces, int F, const float* face_n, const float* edge_n, const float* vert_n,
                         const float* gmin, const float* gmax, int D, int H, int W, int mode, int grid, float* sdf, int* nearest, void* ws,
                         long long ws_bytes, void* stream) {
  return lemo::scene_sdf_build(verts, V, faces, F, face_n, edge_n, vert_n, gmin, gmax, D, H, W, mode, grid, sdf, nearest, ws, ws_bytes,
                               (hipStream_t)stream);
}
}  // extern "C"
