// Which vertices of a body mesh the depth camera sees, for B frames at once: the device form of the reference's
// psbody.mesh.visibility.visibility_compute(v, f, cams) (fitting_temp_slide.py:642-652, a CGAL ray cast per frame on the host) with
// its default min_dist = 1e-3 and neither normals nor sensors.  psbody is not part of this project's environment: the definition
// below is recalled from its source, not confirmed by a run.
//
// Definition.  Frame b, vertex i at p, camera at c: dir = (c - p) / |c - p|, o = p + min_dist dir.  The vertex is VISIBLE iff the
// segment from o to c meets no triangle of that frame's mesh, the triangles incident to i included, from either side (CGAL's
// do_intersect has no facing).  |c - p| <= min_dist (or a length that is not finite) counts as visible.
//
// One predicate, written once (vis_ray, vis_tri, vis_hit).  Every segment of a frame ends at the camera, so the Moeller-Trumbore test
// is taken with the camera as the origin and w = o - c as the direction: the segment is c + t w, 0 <= t <= 1.  With P_k = v_k - c,
// e1 = P1 - P0, e2 = P2 - P0 the quantities of Moeller-Trumbore become
//     det = e1 . (w x e2) = w . (e2 x e1)        u det = -P0 . (w x e2) = w . (P0 x e2)
//     v det = w . (-P0 x e1) = w . (e1 x P0)     t det = e2 . (-P0 x e1) = P0 . (e2 x e1)
// so a triangle is three vectors and a scalar (vis_tri: nd = e2 x e1, a = P0 x e2, q = e1 x P0, tn = P0 . nd) that do not depend on the
// vertex.  The far end of the segment is the one bound that decides the vertex's OWN triangles -- the line through o meets their planes
// at p, min_dist short of o, so t = 1 + min_dist / |w| there -- and t det <= det in the form tn <= w . nd loses that 3e-4 in the
// cancellation of both sides on a triangle seen edge-on.  It is therefore taken as m = (P0 - w) . nd <= 0: P0 - w = v0 - o is the short
// vector from the segment's end to the triangle, and m is |nd| times the signed distance of o from the plane, without cancellation.
// A pair costs four dot products and a vector difference.  Nothing is divided.  The hit rule, inclusive on every bound:
//     det > 0:  U >= 0, V >= 0, U + V <= det, tn >= 0, m <= 0               (U = w . a, V = w . q)
//     det < 0:  U <= 0, V <= 0, U + V >= det, tn <= 0, m >= 0
//     det == 0 (the segment is parallel to the plane, or the triangle is degenerate: nd = 0), or anything that is NaN: no hit.
// fp32 VALU only; every product-sum is an explicit fmaf chain and contraction is off, so a pair has one result whoever evaluates it:
// the host emulator, the brute-force kernel or the binned kernels.  The visibility of a vertex is the AND over all triangles of
// "no hit", hence identical for every acceleration structure, grid size and schedule, bit for bit.
//
// Brute force (any geometry).  The structure of chamfer_nn_kernel: 256 threads, VIS_QPT = 4 vertices per lane in registers (w and a hit
// flag), the frame's triangles set up once per workgroup and streamed through LDS in chunks of VIS_CHUNK = 256 (thirteen floats each, as
// thirteen arrays read at a wave-uniform address), two buffers, one barrier per chunk.  2 x 13 x 256 x 4 B = 26 KB of static LDS.
//
// Binned (frames whose vertices all lie in front of the camera: depth z - c_z >= VIS_ZMIN and |x / z|, |y / z| <= VIS_FOV; any other
// frame silently takes the brute-force path).  The segment of vertex i projects to the single point pi_i = (x / z, y / z) of the
// camera plane, and it can only meet a triangle whose projection contains that point.
//   vis_bin_kernel, one workgroup per frame: bounding box of the pi_i (LDS atomicMax on order-preserving keys), per-cell counts of a
//     G x G grid over it, exclusive scan, fill -- all in LDS.  Writes the frame header, cell_start [G G + 1], cell_items [V] and the
//     directions w in cell order to the caller's workspace.
//   vis_tri_kernel, grid (triangle blocks, frames), one triangle per thread: the cells its projected bounding box overlaps, inflated by
//     VIS_MARGIN on every side, and the predicate against the vertices binned there.  A hit is a plain store of 0 (idempotent).
//   vis_big_kernel: triangles that cover more than VIS_BIG cells, and THIN ones, one workgroup per triangle against every vertex of
//     the frame (depth_raster_big_kernel's scheme).
// Why the inflation is conservative.  grid_cell is monotone in fp32 (geom_device.hpp), so every vertex
// whose pi lies in the inflated box is in a visited cell, exactly.  What has to be covered is where the fp32 predicate can say "hit"
// outside the exact projected triangle.  U, V and det - U - V are the edge functions det[w, P_i, P_j] = w_z P_iz P_jz x (twice the
// signed area of (pi, pi_i, pi_j)); each carries an absolute error of about 2^-20 |w| |P| |e| (two roundings per cross-product term,
// three per dot product; e1 and e2 are differences of nearby points, with a RELATIVE error of 2^-24), so its sign is right once pi is
// farther than some eta = O(2^-20) x (projected edge) x (depth slope of the triangle) from the edge's line, and the three signs can
// agree only within eta / sin(corner / 2) of the triangle.  For a projection that is not THIN (twice its area >= VIS_THIN x the square
// of its longest box side: no corner sharper than about VIS_THIN, depth slope below about 1 / VIS_THIN) and not larger than
// VIS_BIGSIDE that reach is of the order 2^-20 x 2^4 x 2^5 x VIS_BIGSIDE = 2^-13.8, a factor 50 inside VIS_MARGIN = 2^-8.  This is an
// estimate with a wide margin, not a proof to the last constant.  Thin projections (edge-on triangles, slivers) have no bound at all --
// on an exactly edge-on triangle every quantity is rounding noise along the whole extended line -- so they are tested against every
// vertex, like the large ones.  The tests hold brute force and binned to equality on every bit.
#include "geom_device.hpp"
#include "kernels.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace lemo {

#define VIS_BLOCK 256
#define VIS_QPT 4
#define VIS_QPW (VIS_BLOCK * VIS_QPT)                         // vertices per workgroup of the brute-force kernel
#define VIS_CHUNK 256                                        // triangles per LDS buffer
#define VIS_GMAX 64                                          // largest (and default) grid side: G G counters in LDS
#define VIS_BIG 64                                           // a triangle over more cells than this: one workgroup per triangle
#define VIS_ZMIN 0.01f                                       // smallest depth of a frame that is binned
#define VIS_FOV 2.0f                                         // largest |x / z|, |y / z| of a frame that is binned
#define VIS_MARGIN 0.00390625f                               // 2^-8: inflation of a projected bounding box, every side
#define VIS_THIN 0.0625f                                     // 2^-4: twice the projected area below this x (longest box side)^2 = thin
#define VIS_BIGSIDE 0.14359f                                 // 2^-2.8: a projected box side above this goes to the big pass as well
#define VIS_HDR 8                                            // 4-byte words of a frame's header in the workspace

struct VisTri { float nd[3], a[3], q[3], p0[3], tn; };

// w = o - c of the vertex at p; false: |c - p| <= min_dist or not finite (the vertex is visible, nothing is tested)
__device__ __forceinline__ bool vis_ray(const float p[3], const float c[3], float min_dist, float w[3]) {
  const float dx = c[0] - p[0], dy = c[1] - p[1], dz = c[2] - p[2];
  const float len = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
  if (!(len > min_dist) || !(len < GEOM_FMAX)) { w[0] = 0.f; w[1] = 0.f; w[2] = 0.f; return false; }
  const float s = min_dist / len;
  w[0] = fmaf(s, dx, p[0]) - c[0];
  w[1] = fmaf(s, dy, p[1]) - c[1];
  w[2] = fmaf(s, dz, p[2]) - c[2];
  return true;
}

// P_k = v_k - c (already subtracted by the caller with vis_rel) -> the triangle's three vectors and scalar
__device__ __forceinline__ void vis_tri(const float P0[3], const float P1[3], const float P2[3], VisTri& t) {
  float e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { e1[k] = P1[k] - P0[k]; e2[k] = P2[k] - P0[k]; }
  cross3(e2, e1, t.nd);
  cross3(P0, e2, t.a);
  cross3(e1, P0, t.q);
  t.tn = dot3(P0, t.nd);
#pragma unroll
  for (int k = 0; k < 3; ++k) t.p0[k] = P0[k];
}

__device__ __forceinline__ bool vis_hit(const float w[3], const float nd[3], const float a[3], const float q[3], const float p0[3], float tn) {
  const float det = dot3(w, nd), U = dot3(w, a), V = dot3(w, q), S = U + V;
  const float r0 = p0[0] - w[0], r1 = p0[1] - w[1], r2 = p0[2] - w[2];
  const float m = fmaf(r2, nd[2], fmaf(r1, nd[1], r0 * nd[0]));
  const bool pos = det > 0.f && U >= 0.f && V >= 0.f && S <= det && tn >= 0.f && m <= 0.f;
  const bool neg = det < 0.f && U <= 0.f && V <= 0.f && S >= det && tn <= 0.f && m >= 0.f;
  return pos || neg;
}

__device__ __forceinline__ void vis_rel(const float* __restrict__ v, const float c[3], float P[3]) {
  P[0] = v[0] - c[0]; P[1] = v[1] - c[1]; P[2] = v[2] - c[2];
}

// face f of the frame -> setup; a face that names a vertex outside [0, V) never hits (all zeros: det == 0)
__device__ __forceinline__ bool vis_face(const float* __restrict__ vf, int V, const int* __restrict__ faces, int f, const float c[3],
                                         float P0[3], float P1[3], float P2[3], VisTri& t) {
  int id[3];
  const bool ok = face_ids(faces, f, V, id);
  const int i0 = ok ? id[0] : 0, i1 = ok ? id[1] : 0, i2 = ok ? id[2] : 0;      // (vertex 0, vertex 0, vertex 0): degenerate, nd = a = q = 0, det == 0
  vis_rel(vf + 3 * (size_t)i0, c, P0);
  vis_rel(vf + 3 * (size_t)i1, c, P1);
  vis_rel(vf + 3 * (size_t)i2, c, P2);
  vis_tri(P0, P1, P2, t);
  return ok;
}

__device__ __forceinline__ void vis_cam(const float* __restrict__ cam, int b, float c[3]) {
  c[0] = cam ? cam[3 * (size_t)b] : 0.f; c[1] = cam ? cam[3 * (size_t)b + 1] : 0.f; c[2] = cam ? cam[3 * (size_t)b + 2] : 0.f;
}

// ---- brute force -------------------------------------------------------------------------------------------------------------
// grid (vertex block, frame).  hdr: the binned path's frame headers, or NULL; with it a frame whose header says "binned" is left alone
__global__ void __launch_bounds__(VIS_BLOCK) vis_brute_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                              const float* __restrict__ cam, float min_dist, const int* __restrict__ hdr,
                                                              long long hstride, unsigned char* __restrict__ vis) {
  __shared__ __attribute__((aligned(16))) float st[2][13][VIS_CHUNK];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (hdr && hdr[(size_t)b * hstride] == 1) return;           // uniform over the workgroup
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  float c[3];
  vis_cam(cam, b, c);
  const int q0 = blockIdx.x * VIS_QPW + tid;

  float w[VIS_QPT][3];
  bool hit[VIS_QPT];
#pragma unroll
  for (int k = 0; k < VIS_QPT; ++k) {
    const int i = min(q0 + k * VIS_BLOCK, V - 1);             // lanes past the end repeat the last vertex and do not store
    const float p[3] = {vf[3 * (size_t)i], vf[3 * (size_t)i + 1], vf[3 * (size_t)i + 2]};
    vis_ray(p, c, min_dist, w[k]);                            // w = 0 where nothing is to be tested: det == 0 for every triangle
    hit[k] = false;
  }

  VisTri stage;
  auto fetch = [&](int c0) {
    const int f = c0 + tid;
    float P0[3], P1[3], P2[3];
    if (f < F) {
      vis_face(vf, V, faces, f, c, P0, P1, P2, stage);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { stage.nd[k] = 0.f; stage.a[k] = 0.f; stage.q[k] = 0.f; stage.p0[k] = 0.f; }
      stage.tn = 0.f;
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      st[buf][k][tid] = stage.nd[k]; st[buf][3 + k][tid] = stage.a[k]; st[buf][6 + k][tid] = stage.q[k]; st[buf][9 + k][tid] = stage.p0[k];
    }
    st[buf][12][tid] = stage.tn;
  };

  fetch(0);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < F; c0 += VIS_CHUNK, buf ^= 1) {
    const bool more = c0 + VIS_CHUNK < F;
    if (more) fetch(c0 + VIS_CHUNK);
    const int cnt = min(VIS_CHUNK, F - c0);
    for (int j = 0; j < cnt; ++j) {
      const float nd[3] = {st[buf][0][j], st[buf][1][j], st[buf][2][j]};
      const float a[3] = {st[buf][3][j], st[buf][4][j], st[buf][5][j]};
      const float q[3] = {st[buf][6][j], st[buf][7][j], st[buf][8][j]};
      const float p0[3] = {st[buf][9][j], st[buf][10][j], st[buf][11][j]};
      const float tn = st[buf][12][j];
#pragma unroll
      for (int k = 0; k < VIS_QPT; ++k) hit[k] = hit[k] || vis_hit(w[k], nd, a, q, p0, tn);
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }

  unsigned char* __restrict__ o = vis + (size_t)b * V;
#pragma unroll
  for (int k = 0; k < VIS_QPT; ++k) {
    const int i = q0 + k * VIS_BLOCK;
    if (i < V) o[i] = hit[k] ? 0 : 1;
  }
}

// ---- binned ------------------------------------------------------------------------------------------------------------------
// A frame's workspace, laid out from `frame`: hdr [VIS_HDR] ([0] 1 = binned, 0 = brute force; [1..4] x0, y0, sx, sy as float bits),
// cell_start [G G + 1], items [V], wdir [V][3] (floats, in cell order).  P is a pointer to 4-byte words in the kernels, and long long on
// the host, where laying a frame out from word 0 gives its size as `end`.
template <typename P> struct VisWs { P hdr, cell_start, items, wdir, end; };
template <typename P> __host__ __device__ inline VisWs<P> vis_ws(P frame, int V, int G) {
  VisWs<P> w;
  w.hdr = frame; w.cell_start = w.hdr + VIS_HDR; w.items = w.cell_start + (G * G + 1); w.wdir = w.items + V; w.end = w.wdir + 3ll * V;
  return w;
}

// the bins of every frame (NaN never reaches float_key: a vertex that cannot be projected sends the frame to brute force first)
__global__ void __launch_bounds__(VIS_BLOCK) vis_bin_kernel(const float* __restrict__ verts, int V, const float* __restrict__ cam, float min_dist,
                                                            int G, int* __restrict__ ws, long long wstride) {
  __shared__ unsigned s_box[5];                                // max keys of x, -x, y, -y; [4]: a vertex that cannot be projected
  __shared__ int s_cnt[VIS_GMAX * VIS_GMAX];
  __shared__ int s_part[VIS_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x, nc = G * G;
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  const VisWs<int*> fr = vis_ws(ws + (size_t)b * wstride, V, G);
  int* __restrict__ hdr = fr.hdr;
  float* __restrict__ wdir = reinterpret_cast<float*>(fr.wdir);
  float c[3];
  vis_cam(cam, b, c);
  if (tid < 5) s_box[tid] = 0u;
  for (int k = tid; k < nc; k += VIS_BLOCK) s_cnt[k] = 0;
  __syncthreads();

  unsigned kx1 = 0u, kx0 = 0u, ky1 = 0u, ky0 = 0u, bad = 0u;
  for (int i = tid; i < V; i += VIS_BLOCK) {
    float P[3];
    vis_rel(vf + 3 * (size_t)i, c, P);
    const float x = P[0] / P[2], y = P[1] / P[2];
    if (!(P[2] >= VIS_ZMIN) || !(fabsf(x) <= VIS_FOV) || !(fabsf(y) <= VIS_FOV)) { bad = 1u; continue; }
    kx1 = max(kx1, float_key(x)); kx0 = max(kx0, float_key(-x));
    ky1 = max(ky1, float_key(y)); ky0 = max(ky0, float_key(-y));
  }
  if (kx1) { atomicMax(&s_box[0], kx1); atomicMax(&s_box[1], kx0); atomicMax(&s_box[2], ky1); atomicMax(&s_box[3], ky0); }
  if (bad) atomicMax(&s_box[4], 1u);
  __syncthreads();
  if (s_box[4] || !s_box[0]) {                                 // uniform: the frame goes to the brute-force kernel
    if (tid == 0) hdr[0] = 0;
    return;
  }
  const float x1 = float_unkey(s_box[0]), x0 = -float_unkey(s_box[1]), y1 = float_unkey(s_box[2]), y0 = -float_unkey(s_box[3]);
  const float ex = x1 - x0, ey = y1 - y0;
  const float sx = ex > 0.f ? (float)G / ex : 0.f, sy = ey > 0.f ? (float)G / ey : 0.f;
  if (tid == 0) {
    hdr[0] = 1;
    hdr[1] = __float_as_int(x0); hdr[2] = __float_as_int(y0); hdr[3] = __float_as_int(sx); hdr[4] = __float_as_int(sy);
  }

  for (int i = tid; i < V; i += VIS_BLOCK) {
    float P[3];
    vis_rel(vf + 3 * (size_t)i, c, P);
    const int cell = grid_cell(P[1] / P[2], y0, sy, G) * G + grid_cell(P[0] / P[2], x0, sx, G);
    atomicAdd(&s_cnt[cell], 1);
  }
  __syncthreads();
  // exclusive scan of the nc <= 4096 counters; s_cnt becomes the fill cursor
  block_exclusive_scan<VIS_BLOCK>(nc, s_part, [&](int k) { return s_cnt[k]; }, [&](int k, int acc) { s_cnt[k] = acc; fr.cell_start[k] = acc; });
  if (tid == 0) fr.cell_start[nc] = V;
  __syncthreads();
  for (int i = tid; i < V; i += VIS_BLOCK) {
    float P[3], w[3];
    const float p[3] = {vf[3 * (size_t)i], vf[3 * (size_t)i + 1], vf[3 * (size_t)i + 2]};
    vis_rel(p, c, P);
    const int cell = grid_cell(P[1] / P[2], y0, sy, G) * G + grid_cell(P[0] / P[2], x0, sx, G);
    const int slot = atomicAdd(&s_cnt[cell], 1);
    vis_ray(p, c, min_dist, w);
    fr.items[slot] = i;
    wdir[3 * (size_t)slot] = w[0]; wdir[3 * (size_t)slot + 1] = w[1]; wdir[3 * (size_t)slot + 2] = w[2];
  }
}

struct VisBox { int lx, hx, ly, hy; bool big; };

// the cells a triangle has to visit, or big = true: more than VIS_BIG of them, a thin projection, or a box side above VIS_BIGSIDE
__device__ __forceinline__ void vis_box(const float P0[3], const float P1[3], const float P2[3], const int* __restrict__ hdr, int G, VisBox& o) {
  const float x0 = __int_as_float(hdr[1]), y0 = __int_as_float(hdr[2]), sx = __int_as_float(hdr[3]), sy = __int_as_float(hdr[4]);
  const float ax = P0[0] / P0[2], ay = P0[1] / P0[2], bx = P1[0] / P1[2], by = P1[1] / P1[2], cx = P2[0] / P2[2], cy = P2[1] / P2[2];
  const float xmin = fminf(ax, fminf(bx, cx)), xmax = fmaxf(ax, fmaxf(bx, cx));
  const float ymin = fminf(ay, fminf(by, cy)), ymax = fmaxf(ay, fmaxf(by, cy));
  o.lx = grid_cell(xmin - VIS_MARGIN, x0, sx, G); o.hx = grid_cell(xmax + VIS_MARGIN, x0, sx, G);
  o.ly = grid_cell(ymin - VIS_MARGIN, y0, sy, G); o.hy = grid_cell(ymax + VIS_MARGIN, y0, sy, G);
  const float side = fmaxf(xmax - xmin, ymax - ymin);
  const float area2 = fabsf(fmaf(bx - ax, cy - ay, -((cx - ax) * (by - ay))));
  const bool thin = !(area2 >= VIS_THIN * (side * side));      // also a projection that is not finite
  o.big = thin || !(side <= VIS_BIGSIDE) || (o.hx - o.lx + 1) * (o.hy - o.ly + 1) > VIS_BIG;
}

// grid (triangle block, frame): one triangle per thread against the vertices binned under its inflated box
__global__ void __launch_bounds__(VIS_BLOCK) vis_tri_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                            const float* __restrict__ cam, int G, const int* __restrict__ ws, long long wstride,
                                                            unsigned char* __restrict__ vis) {
  const int b = blockIdx.y, f = blockIdx.x * VIS_BLOCK + threadIdx.x;
  const VisWs<const int*> fr = vis_ws(ws + (size_t)b * wstride, V, G);
  const int* __restrict__ hdr = fr.hdr;
  if (hdr[0] != 1 || f >= F) return;
  const float* __restrict__ wdir = reinterpret_cast<const float*>(fr.wdir);
  float c[3], P0[3], P1[3], P2[3];
  vis_cam(cam, b, c);
  VisTri t;
  if (!vis_face(verts + (size_t)b * V * 3, V, faces, f, c, P0, P1, P2, t)) return;
  VisBox box;
  vis_box(P0, P1, P2, hdr, G, box);
  if (box.big) return;
  unsigned char* __restrict__ o = vis + (size_t)b * V;
  for (int cy = box.ly; cy <= box.hy; ++cy) {
    const int s0 = fr.cell_start[cy * G + box.lx], s1 = fr.cell_start[cy * G + box.hx + 1];       // the cells of one row are contiguous
    for (int s = s0; s < s1; ++s) {
      const float w[3] = {wdir[3 * (size_t)s], wdir[3 * (size_t)s + 1], wdir[3 * (size_t)s + 2]};
      if (vis_hit(w, t.nd, t.a, t.q, t.p0, t.tn)) o[fr.items[s]] = 0;
    }
  }
}

// the big and thin triangles of every block of VIS_BLOCK, one at a time with all threads, against every vertex of the frame
__global__ void __launch_bounds__(VIS_BLOCK) vis_big_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                            const float* __restrict__ cam, int G, const int* __restrict__ ws, long long wstride,
                                                            unsigned char* __restrict__ vis, int* __restrict__ nbig) {
  __shared__ int list[VIS_BLOCK];
  __shared__ int count;
  const int tid = threadIdx.x, b = blockIdx.y, f = blockIdx.x * VIS_BLOCK + tid;
  const VisWs<const int*> fr = vis_ws(ws + (size_t)b * wstride, V, G);
  const int* __restrict__ hdr = fr.hdr;
  if (hdr[0] != 1) return;                                    // uniform
  const float* __restrict__ wdir = reinterpret_cast<const float*>(fr.wdir);
  const float* __restrict__ vf = verts + (size_t)b * V * 3;
  float c[3], P0[3], P1[3], P2[3];
  vis_cam(cam, b, c);
  if (tid == 0) count = 0;
  __syncthreads();
  VisTri t;
  if (f < F && vis_face(vf, V, faces, f, c, P0, P1, P2, t)) {
    VisBox box;
    vis_box(P0, P1, P2, hdr, G, box);
    if (box.big) list[atomicAdd(&count, 1)] = f;
  }
  __syncthreads();
  const int n = count;
  if (nbig && tid == 0 && n) atomicAdd(&nbig[b], n);
  unsigned char* __restrict__ o = vis + (size_t)b * V;
  for (int i = 0; i < n; ++i) {
    vis_face(vf, V, faces, list[i], c, P0, P1, P2, t);
    for (int s = tid; s < V; s += VIS_BLOCK) {
      const float w[3] = {wdir[3 * (size_t)s], wdir[3 * (size_t)s + 1], wdir[3 * (size_t)s + 2]};
      if (vis_hit(w, t.nd, t.a, t.q, t.p0, t.tn)) o[fr.items[s]] = 0;
    }
  }
}

namespace {

int vis_shape(int B, int V, int F, int mode, int grid) {
  if (mode < LEMO_VIS_AUTO || mode > LEMO_VIS_BINNED) return LEMO_ERR_ARG;
  if (grid < 0 || grid == 1 || grid > VIS_GMAX) return LEMO_ERR_ARG;
  if (B < 1 || V < 1 || F < 1 || B > 65535 || F > (1 << 30) || (long long)B * V > (1ll << 30)) return LEMO_ERR_SHAPE;
  return 0;
}

long long vis_words(int V, int G) { return vis_ws(0ll, V, G).end; }

// what `auto` means: profiles/scan_terms_rate.txt decides
#define VIS_AUTO_MODE LEMO_VIS_BINNED

}  // namespace

long long vertex_visibility_workspace_bytes(int B, int V, int F, int mode, int grid) {
  if (vis_shape(B, V, F, mode, grid)) return -1;
  if (mode == LEMO_VIS_AUTO) mode = VIS_AUTO_MODE;
  if (mode == LEMO_VIS_BRUTE) return 0;
  return 4 * (long long)B * vis_words(V, grid ? grid : VIS_GMAX);
}

int vertex_visibility(const float* verts, int B, int V, const int* faces, int F, const float* cam, float min_dist, int mode, int grid,
                      unsigned char* vis, int* nbig, void* ws, long long ws_bytes, hipStream_t s) {
  if (int e = vis_shape(B, V, F, mode, grid)) return e;
  if (!verts || !faces || !vis || ws_bytes < 0 || !(min_dist >= 0.f) || !std::isfinite(min_dist)) return LEMO_ERR_ARG;
  if (mode == LEMO_VIS_AUTO) mode = VIS_AUTO_MODE;
  const dim3 blk(VIS_BLOCK), gv((V + VIS_QPW - 1) / VIS_QPW, B), gf((F + VIS_BLOCK - 1) / VIS_BLOCK, B);
  if (nbig) if (hipError_t e = hipMemsetAsync(nbig, 0, (size_t)B * sizeof(int), s)) return (int)e;
  if (mode == LEMO_VIS_BRUTE) {
    hipLaunchKernelGGL(vis_brute_kernel, gv, blk, 0, s, verts, V, faces, F, cam, min_dist, (const int*)nullptr, 0ll, vis);
    return (int)hipGetLastError();
  }
  const int G = grid ? grid : VIS_GMAX;
  const long long words = vis_words(V, G);
  if (!ws || ws_bytes < 4 * (long long)B * words) return LEMO_ERR_ARG;
  int* w = static_cast<int*>(ws);
  if (hipError_t e = hipMemsetAsync(vis, 1, (size_t)B * V, s)) return (int)e;                  // a hit stores 0
  hipLaunchKernelGGL(vis_bin_kernel, dim3(B), blk, 0, s, verts, V, cam, min_dist, G, w, words);
  hipLaunchKernelGGL(vis_tri_kernel, gf, blk, 0, s, verts, V, faces, F, cam, G, (const int*)w, words, vis);
  hipLaunchKernelGGL(vis_big_kernel, gf, blk, 0, s, verts, V, faces, F, cam, G, (const int*)w, words, vis, nbig);
  hipLaunchKernelGGL(vis_brute_kernel, gv, blk, 0, s, verts, V, faces, F, cam, min_dist, (const int*)w, words, vis);   // frames the bins refused
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
long long lemo_vertex_visibility_workspace_bytes(int B, int V, int F, int mode, int grid) {
  return lemo::vertex_visibility_workspace_bytes(B, V, F, mode, grid);
}
int lemo_vertex_visibility(const float* verts, int B, int V, const int* faces, int F, const float* cam, float min_dist, int mode, int grid,
                           unsigned char* vis, int* nbig, void* ws, long long ws_bytes, void* stream) {
  return lemo::vertex_visibility(verts, B, V, faces, F, cam, min_dist, mode, grid, vis, nbig, ws, ws_bytes, (hipStream_t)stream);
}
}  // extern "C"
