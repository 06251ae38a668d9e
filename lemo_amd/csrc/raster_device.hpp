// The raster's device functions, shared by occlusion_kernels.hip (depth raster, per-point query), render_kernels.hip (batched
// depth, face ids, shading) and view_kernels.hip (scene views): ONE oc_setup / oc_key pair, so a depth one of them computes is bit
// for bit the other's, and ONE shading function (rn_shade_bary), so a body pixel has the same colour in an overlay and in a view.
//
// Geometry.  Camera space is y down, z forward; pixel [y][x] samples the ray d = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1).
// Coverage uses homogeneous edge functions e_i = d . (p_j x (p_k - p_j)): the ray meets the triangle's plane inside the triangle
// iff the three have one sign.  They need no projected vertex, so a triangle that crosses the near plane or reaches behind the
// camera is handled per pixel without clipping.  Depth is the ray-plane intersection Z = (n . p0) / (n . d), n = (p1 - p0) x (p2 - p0);
// a hit counts iff znear <= Z <= zfar.  The nearest hit wins through atomicMax on the key 0xFFFFFFFF - float_bits(Z) (Z > 0: the bit
// patterns order like the values; 0 = no hit), which makes every image independent of the order of faces, threads and launches.
// fp32 VALU only, no fused multiply-adds the source does not spell out (the tests hold the kernels to a float32 numpy restatement
// operation by operation).
#pragma once
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace lemo {

#define OC_BLOCK 256
#define OC_MAXP 128                                          // query points per frame (LDS staging)
#define OC_BIG 256                                           // bounding boxes above this many pixels: one workgroup per triangle
#define OC_FPT 4                                             // faces per thread of the query
#define OC_NOPIX (-2147483647 - 1)                           // pixel index of a projection that is not finite (numpy's astype(int))

struct OcCam {
  float fx, fy, cx, cy, znear, zfar;
  int W, H, cull;
};
struct OcXf { float m[12]; int on; };                        // [R | t] row-major, applied on load

struct OcTri {
  float e0[3], e1[3], e2[3], n[3], D;
  int x0, x1, y0, y1;                                        // bounding box, clamped to the image
};

__device__ __forceinline__ void oc_cross(const float a[3], const float b[3], float c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void oc_load(const float* __restrict__ v, const OcXf& X, float p[3]) {
  const float x = v[0], y = v[1], z = v[2];
  if (!X.on) { p[0] = x; p[1] = y; p[2] = z; return; }
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ((X.m[4 * k] * x + X.m[4 * k + 1] * y) + X.m[4 * k + 2] * z) + X.m[4 * k + 3];
}

__device__ __forceinline__ float oc_ray_x(int x, const OcCam& c) { return (((float)x + 0.5f) - c.cx) / c.fx; }
__device__ __forceinline__ float oc_ray_y(int y, const OcCam& c) { return (((float)y + 0.5f) - c.cy) / c.fy; }

// lower / upper pixel bound of a projected interval [lo, hi], one pixel wider on either side, clamped to [0, n - 1]
__device__ __forceinline__ void oc_span(float lo, float hi, int n, int& a, int& b) {
  a = (int)fminf(fmaxf(floorf(lo) - 1.0f, 0.0f), (float)n);
  b = (int)fminf(fmaxf(floorf(hi) + 1.0f, -1.0f), (float)(n - 1));
}

// false: nothing of the triangle can be drawn (culled, outside the depth range or the image, not finite)
__device__ __forceinline__ bool oc_setup(const float p0[3], const float p1[3], const float p2[3], const OcCam& c, OcTri& t) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && fabsf(p0[k]) < 3.0e38f && fabsf(p1[k]) < 3.0e38f && fabsf(p2[k]) < 3.0e38f;
  if (!fin) return false;
  float a[3], b[3], g[3], d2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = p1[k] - p0[k]; b[k] = p2[k] - p1[k]; g[k] = p0[k] - p2[k]; d2[k] = p2[k] - p0[k]; }
  oc_cross(p1, b, t.e0);
  oc_cross(p2, g, t.e1);
  oc_cross(p0, a, t.e2);
  oc_cross(a, d2, t.n);
  t.D = (t.n[0] * p0[0] + t.n[1] * p0[1]) + t.n[2] * p0[2];
  if (c.cull && !(t.D < 0.0f)) return false;                  // counter-clockwise as the camera sees it, or not drawn
  const float zmin = fminf(p0[2], fminf(p1[2], p2[2])), zmax = fmaxf(p0[2], fmaxf(p1[2], p2[2]));
  if (zmax < c.znear || zmin > c.zfar) return false;
  if (zmin >= c.znear) {
    const float u0 = (c.fx * p0[0]) / p0[2] + c.cx, u1 = (c.fx * p1[0]) / p1[2] + c.cx, u2 = (c.fx * p2[0]) / p2[2] + c.cx;
    const float v0 = (c.fy * p0[1]) / p0[2] + c.cy, v1 = (c.fy * p1[1]) / p1[2] + c.cy, v2 = (c.fy * p2[1]) / p2[2] + c.cy;
    oc_span(fminf(u0, fminf(u1, u2)), fmaxf(u0, fmaxf(u1, u2)), c.W, t.x0, t.x1);
    oc_span(fminf(v0, fminf(v1, v2)), fmaxf(v0, fmaxf(v1, v2)), c.H, t.y0, t.y1);
  } else {                                                    // crosses the near plane: its projection is unbounded, every pixel is tested
    t.x0 = 0; t.x1 = c.W - 1; t.y0 = 0; t.y1 = c.H - 1;
  }
  return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// key of the hit of ray (dx, dy, 1) on the triangle, 0 without one
__device__ __forceinline__ unsigned oc_key(const OcTri& t, float dx, float dy, const OcCam& c) {
  const float e0 = (t.e0[0] * dx + t.e0[1] * dy) + t.e0[2];
  const float e1 = (t.e1[0] * dx + t.e1[1] * dy) + t.e1[2];
  const float e2 = (t.e2[0] * dx + t.e2[1] * dy) + t.e2[2];
  const bool in = (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
  if (!in) return 0u;
  const float nd = (t.n[0] * dx + t.n[1] * dy) + t.n[2];
  const float Z = t.D / nd;
  if (!(Z >= c.znear && Z <= c.zfar)) return 0u;               // also a NaN of a degenerate triangle
  return 0xFFFFFFFFu - __float_as_uint(Z);
}

__device__ __forceinline__ float oc_depth(unsigned key) { return key ? __uint_as_float(0xFFFFFFFFu - key) : 0.0f; }

// face f of the mesh -> setup; false also for a face that names a vertex the mesh does not have
__device__ __forceinline__ bool oc_face(const float* __restrict__ verts, int V, const int* __restrict__ faces, int f, const OcXf& X,
                                        const OcCam& c, OcTri& t) {
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  float p0[3], p1[3], p2[3];
  oc_load(verts + 3 * (size_t)i0, X, p0);
  oc_load(verts + 3 * (size_t)i1, X, p1);
  oc_load(verts + 3 * (size_t)i2, X, p2);
  return oc_setup(p0, p1, p2, c, t);
}

__device__ __forceinline__ bool oc_is_big(const OcTri& t) { return (t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > OC_BIG; }

// ---- shading, shared by render_kernels.hip (body overlays) and view_kernels.hip (scene views): ONE function, the same bits ------
struct RnShade { float base[3], ambient, diffuse; };

// (int)(255 c + 0.5) clamped to 0 .. 255 (a NaN gives 0)
__device__ __forceinline__ unsigned rn_quant(float c) { return (unsigned)(int)fminf(fmaxf(255.0f * c + 0.5f, 0.0f), 255.0f); }

// shade of pixel (x, y) under face f of one frame (rule 3 of lemo_amd/render.py); bw: the perspective-correct weights of the face's
// three vertices at the pixel's ray (0 for a face that cannot be drawn); lit = false: shade 1, the weights only
__device__ __forceinline__ float rn_shade_bary(const float* __restrict__ vf, const float* __restrict__ nf, int V, const int* __restrict__ faces,
                                               int f, const OcCam& c, float ambient, float diffuse, bool lit, int x, int y, float bw[3]) {
  OcXf X = {};
  OcTri t;
  float lam = 0.0f;
  bw[0] = bw[1] = bw[2] = 0.0f;
  if (oc_face(vf, V, faces, f, X, c, t)) {                    // true for every id the id pass wrote
    const float dx = oc_ray_x(x, c), dy = oc_ray_y(y, c);
    const float e0 = (t.e0[0] * dx + t.e0[1] * dy) + t.e0[2];
    const float e1 = (t.e1[0] * dx + t.e1[1] * dy) + t.e1[2];
    const float e2 = (t.e2[0] * dx + t.e2[1] * dy) + t.e2[2];
    const float s = (e0 + e1) + e2;
    const float b0 = e0 / s, b1 = e1 / s, b2 = e2 / s;
    bw[0] = b0; bw[1] = b1; bw[2] = b2;
    if (!lit) return 1.0f;
    const float *n0 = nf + 3 * (size_t)faces[3 * (size_t)f], *n1 = nf + 3 * (size_t)faces[3 * (size_t)f + 1],
                *n2 = nf + 3 * (size_t)faces[3 * (size_t)f + 2];
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (b0 * n0[k] + b1 * n1[k]) + b2 * n2[k];
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len > 0.0f) lam = fabsf(n[2]) / len;                  // false also for a NaN
  }
  if (!lit) return 1.0f;
  return fminf(1.0f, ambient + diffuse * lam);
}

__device__ __forceinline__ float rn_shade(const float* __restrict__ vf, const float* __restrict__ nf, int V, const int* __restrict__ faces, int f,
                                          const OcCam& c, const RnShade& sh, int x, int y) {
  float bw[3];
  return rn_shade_bary(vf, nf, V, faces, f, c, sh.ambient, sh.diffuse, true, x, y, bw);
}

// the C ABI's camera, validated -> the kernels' (LEMO_ERR_SHAPE / LEMO_ERR_ARG as include/lemo_hip.h documents)
static inline int oc_cam(const lemo_occl_cam* cam, OcCam& c) {
  if (!cam) return LEMO_ERR_ARG;
  if (cam->W < 1 || cam->H < 1 || cam->W > 32768 || cam->H > 32768) return LEMO_ERR_SHAPE;
  if (!(cam->fx > 0.f) || !(cam->fy > 0.f) || !std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) ||
      !std::isfinite(cam->cy) || !(cam->znear > 0.f) || !(cam->zfar >= cam->znear) || !std::isfinite(cam->zfar))
    return LEMO_ERR_ARG;
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy; c.znear = cam->znear; c.zfar = cam->zfar;
  c.W = cam->W; c.H = cam->H; c.cull = cam->cull_backface ? 1 : 0;
  return 0;
}

}  // namespace lemo
