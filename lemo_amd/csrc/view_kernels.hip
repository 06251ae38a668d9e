// 3-D views of fitted bodies on the device: what the reference's temp_prox/renderer.py ('3d' mode), temp_prox/viz/viz_fitting.py and
// vis_opt_amass.py show with pyrender / open3d on the host -- the body inside the coloured scene mesh, its markers as spheres -- as
//     view_transform_kernel      points through [R | t] (oc_load's formula) into a workspace; lemo_vertex_normals and lemo_render_ids
//                                then run on that workspace, for the scene (once per view) and for the bodies (per chunk of frames)
//     view_scene_resolve_kernel  the static layer of one view: per covered pixel the interpolated vertex colour times the shade
//     view_compose_kernel        the per-frame pass, one launch over (tile, frame): the body's key and id, the static key and rgb,
//                                the nearest analytic sphere hit -> owner -> rgb (+ depth, owner); the body is shaded only where it wins
// The rules are written out in lemo_amd/scene_view.py.  The shading is rn_shade_bary of raster_device.hpp, the function the body
// overlays shade with.  fp32 VALU with every operation spelled out (no contraction): the tests hold the kernels to a float32 numpy
// restatement operation by operation.
#include "raster_device.hpp"

#include <cstdint>

#pragma clang fp contract(off)

namespace lemo {

#define VW_PPT 4                                             // pixels per thread: 12 bytes = 3 dwords of uint8 rgb
#define VW_TW 64                                             // tile: 16 threads x VW_PPT pixels wide,
#define VW_TH 16                                             //       16 rows high = OC_BLOCK threads
#define VW_MAXP 256                                          // spheres per frame: one per thread of the cull

struct VwArgs {
  const float *verts, *normals;                              // the body in camera space [B][V][3]
  const int* faces;
  int V, F;
  const unsigned *keys, *ids;                                // the body's [B][H][W], as lemo_render_ids wrote them
  const unsigned* scene_key;                                 // [H][W] or null
  const unsigned char* scene_rgb;                            // [H][W][3]
  const float *spheres, *radius;                             // [B][P][3] world, [P]
  const unsigned char* sphere_rgb;                           // [P][3] or [B][P][3]
  int P, rgb_shared;
  OcXf X;                                                    // world -> camera for the sphere centres
  RnShade sh;
  unsigned bg;                                               // r | g << 8 | b << 16
  unsigned char* rgb;
  float* depth;
  int* owner;
  int p0;                                                    // (address of rgb) mod 4
};

__global__ void __launch_bounds__(OC_BLOCK) view_transform_kernel(const float* __restrict__ pts, size_t n, OcXf X, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= n) return;
  float p[3];
  oc_load(pts + 3 * i, X, p);
  out[3 * i] = p[0]; out[3 * i + 1] = p[1]; out[3 * i + 2] = p[2];
}

__device__ __forceinline__ float vw_unit(unsigned char v) { return (float)v / 255.0f; }

// one thread per pixel of the static layer (rule 2 of lemo_amd/scene_view.py); runs once per view
__global__ void __launch_bounds__(OC_BLOCK) view_scene_resolve_kernel(const float* __restrict__ verts, const float* __restrict__ normals, int V,
                                                                      const int* __restrict__ faces, int F, OcCam c, const unsigned* __restrict__ ids,
                                                                      const unsigned char* __restrict__ colors, float ambient, float diffuse, int lit,
                                                                      unsigned char* __restrict__ rgb) {
  const size_t i = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= (size_t)c.W * c.H) return;
  const unsigned id = ids[i];
  unsigned q[3] = {0u, 0u, 0u};
  if (id != 0u && 0xFFFFFFFFu - id < (unsigned)F) {
    const int f = (int)(0xFFFFFFFFu - id), y = (int)(i / (unsigned)c.W), x = (int)(i - (size_t)y * c.W);
    float bw[3];
    const float shade = rn_shade_bary(verts, normals, V, faces, f, c, ambient, diffuse, lit != 0, x, y, bw);
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float col = (bw[0] * vw_unit(colors[3 * (size_t)i0 + k]) + bw[1] * vw_unit(colors[3 * (size_t)i1 + k])) +
                          bw[2] * vw_unit(colors[3 * (size_t)i2 + k]);
        q[k] = rn_quant(col * shade);
      }
    }
  }
  rgb[3 * i] = (unsigned char)q[0]; rgb[3 * i + 1] = (unsigned char)q[1]; rgb[3 * i + 2] = (unsigned char)q[2];
}

// key of the hit of ray (dx, dy, 1) on the sphere (centre c, squared radius r2), 0 without one (rule 4)
__device__ __forceinline__ unsigned vw_sphere_key(const float c[3], float r2, float dx, float dy, const OcCam& cam) {
  const float d[3] = {dx, dy, 1.0f};
  const float A = (dx * dx + dy * dy) + 1.0f;
  float q[3];
  oc_cross(c, d, q);
  const float disc = A * r2 - ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  if (!(disc >= 0.0f)) return 0u;
  const float Z = (((dx * c[0] + dy * c[1]) + c[2]) - sqrtf(disc)) / A;
  if (!(Z >= cam.znear && Z <= cam.zfar)) return 0u;
  return 0xFFFFFFFFu - __float_as_uint(Z);
}

// grid (tiles in x, tiles in y, B).  A workgroup owns VW_TH rows of VW_TW pixels.  Row y of the tile starts at X0 - shift(y), shift in
// 0 .. 3 chosen so that every thread's four pixels begin on a dword of rgb, whatever W is and wherever in a larger tensor the frames
// start; the groups that stick out of the row on either side go byte by byte.  The launcher sizes the grid so that the shifted tiles
// still reach the end of every row.
__global__ void __launch_bounds__(OC_BLOCK) view_compose_kernel(VwArgs a, OcCam c) {
  __shared__ float s_c[VW_MAXP][4];
  __shared__ int s_idx[VW_MAXP];
  __shared__ int s_flag[VW_MAXP];
  __shared__ int s_n;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int X0 = blockIdx.x * VW_TW, Y0 = blockIdx.y * VW_TH;
  int n = 0;
  if (a.P > 0) {
    // the frame's spheres that can reach this tile, in index order: a conservative bound from the box [c - r, c + r], one pixel wider
    float sc[3] = {0.0f, 0.0f, 0.0f}, r = 0.0f;
    bool ok = false;
    if (tid < a.P) {
      oc_load(a.spheres + ((size_t)b * a.P + tid) * 3, a.X, sc);
      r = a.radius[tid];
      ok = fabsf(sc[0]) < 3.0e38f && fabsf(sc[1]) < 3.0e38f && fabsf(sc[2]) < 3.0e38f && r < 3.0e38f && r > 0.0f && !(sc[2] - r < c.znear);
      if (ok) {
        const float zn = sc[2] - r, zf = sc[2] + r;            // zn >= znear > 0
        const float xl = sc[0] - r, xh = sc[0] + r, yl = sc[1] - r, yh = sc[1] + r;
        const float ulo = c.fx * (xl < 0.0f ? xl / zn : xl / zf) + c.cx, uhi = c.fx * (xh > 0.0f ? xh / zn : xh / zf) + c.cx;
        const float vlo = c.fy * (yl < 0.0f ? yl / zn : yl / zf) + c.cy, vhi = c.fy * (yh > 0.0f ? yh / zn : yh / zf) + c.cy;
        int x0, x1, y0, y1;
        oc_span(ulo, uhi, c.W, x0, x1);
        oc_span(vlo, vhi, c.H, y0, y1);
        ok = x0 <= x1 && y0 <= y1 && x1 >= X0 - (VW_PPT - 1) && x0 < X0 + VW_TW && y1 >= Y0 && y0 < Y0 + VW_TH;
      }
      s_flag[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid < a.P && (ok || tid == a.P - 1)) {
      int pos = 0;
      for (int k = 0; k < tid; ++k) pos += s_flag[k];
      if (ok) { s_c[pos][0] = sc[0]; s_c[pos][1] = sc[1]; s_c[pos][2] = sc[2]; s_c[pos][3] = r * r; s_idx[pos] = tid; }
      if (tid == a.P - 1) s_n = pos + (ok ? 1 : 0);
    }
    __syncthreads();
    n = s_n;
  }
  const int y = Y0 + tid / (VW_TW / VW_PPT);
  if (y >= c.H) return;
  const size_t HW = (size_t)c.W * c.H, row = ((size_t)b * c.H + y) * c.W;
  const int shift = (int)((row + 4 - (size_t)a.p0) & 3);
  const int xs = X0 + VW_PPT * (tid % (VW_TW / VW_PPT)) - shift;
  if (xs >= c.W || xs + VW_PPT <= 0) return;
  const bool full = xs >= 0 && xs + VW_PPT <= c.W;
  const float dy = oc_ray_y(y, c);
  unsigned col[VW_PPT] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < VW_PPT; ++j) {
    const int x = xs + j;
    if (x < 0 || x >= c.W) continue;
    const size_t pix = (size_t)y * c.W + x, gi = (size_t)b * HW + pix;
    const unsigned id = a.ids[gi];
    const bool body = id != 0u && 0xFFFFFFFFu - id < (unsigned)a.F;
    const unsigned kb = body ? a.keys[gi] : 0u;
    const unsigned kc = a.scene_key ? a.scene_key[pix] : 0u;
    unsigned ks = 0u;
    int si = 0;
    const float dx = oc_ray_x(x, c);
    for (int i = 0; i < n; ++i) {
      const unsigned k = vw_sphere_key(s_c[i], s_c[i][3], dx, dy, c);
      if (k > ks) { ks = k; si = i; }                         // equal keys: the lowest index stays
    }
    // the nearest wins; on equal keys the body, then the spheres, then the scene (rule 5)
    int own = -1;
    unsigned key = 0u;
    if (kb != 0u && kb >= ks && kb >= kc) {
      own = 1; key = kb;
      const float shade = rn_shade(a.verts + (size_t)b * a.V * 3, a.normals + (size_t)b * a.V * 3, a.V, a.faces, (int)(0xFFFFFFFFu - id), c, a.sh, x, y);
      col[j] = rn_quant(a.sh.base[0] * shade) | (rn_quant(a.sh.base[1] * shade) << 8) | (rn_quant(a.sh.base[2] * shade) << 16);
    } else if (ks != 0u && ks >= kc) {
      const int s = s_idx[si];
      own = 2 + s; key = ks;
      const float Z = oc_depth(ks);
      const float n0 = Z * dx - s_c[si][0], n1 = Z * dy - s_c[si][1], n2 = Z - s_c[si][2];
      const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
      float lam = 0.0f;
      if (len > 0.0f) lam = fabsf(n2) / len;
      const float shade = fminf(1.0f, a.sh.ambient + a.sh.diffuse * lam);
      const unsigned char* sc = a.sphere_rgb + ((a.rgb_shared ? (size_t)0 : (size_t)b * a.P) + s) * 3;
      col[j] = rn_quant(vw_unit(sc[0]) * shade) | (rn_quant(vw_unit(sc[1]) * shade) << 8) | (rn_quant(vw_unit(sc[2]) * shade) << 16);
    } else if (kc != 0u) {
      own = 0; key = kc;
      const unsigned char* sr = a.scene_rgb + 3 * pix;
      col[j] = sr[0] | (sr[1] << 8) | (sr[2] << 16);
    } else {
      col[j] = a.bg;
    }
    if (a.depth) a.depth[gi] = oc_depth(key);
    if (a.owner) a.owner[gi] = own;
    if (!full) { a.rgb[3 * gi] = (unsigned char)col[j]; a.rgb[3 * gi + 1] = (unsigned char)(col[j] >> 8); a.rgb[3 * gi + 2] = (unsigned char)(col[j] >> 16); }
  }
  if (full) {
    unsigned* w = (unsigned*)(a.rgb + 3 * (row + (size_t)xs));
    w[0] = col[0] | (col[1] << 24);
    w[1] = (col[1] >> 8) | (col[2] << 16);
    w[2] = (col[2] >> 16) | (col[3] << 8);
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static void vw_xf(const float* xf, OcXf& X) {
  X.on = xf ? 1 : 0;
  for (int k = 0; k < 12; ++k) X.m[k] = xf ? xf[k] : 0.0f;
}

int view_transform(const float* points, long long n, const float* xf, float* out, hipStream_t s) {
  if (!points || !out || !xf) return LEMO_ERR_ARG;
  if (n < 1 || n > (1ll << 30)) return LEMO_ERR_SHAPE;
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(xf[k])) return LEMO_ERR_ARG;
  OcXf X;
  vw_xf(xf, X);
  hipLaunchKernelGGL(view_transform_kernel, dim3((unsigned)((n + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s, points, (size_t)n, X, out);
  return (int)hipGetLastError();
}

static bool vw_unit_ok(float v) { return v >= 0.f && v <= 1.f; }

int view_scene_resolve(const float* verts, const float* normals, int V, const int* faces, int F, const lemo_occl_cam* cam, const unsigned* ids,
                       const unsigned char* colors, float ambient, float diffuse, int lit, unsigned char* rgb, hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || (lit && !normals) || !faces || !ids || !colors || !rgb) return LEMO_ERR_ARG;
  if (!vw_unit_ok(ambient) || !vw_unit_ok(diffuse)) return LEMO_ERR_ARG;
  if (V < 1 || V > (1 << 30) || F < 1 || F > (1 << 30)) return LEMO_ERR_SHAPE;
  const size_t n = (size_t)c.W * c.H;
  hipLaunchKernelGGL(view_scene_resolve_kernel, dim3((unsigned)((n + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s, verts, normals, V, faces, F, c,
                     ids, colors, ambient, diffuse, lit ? 1 : 0, rgb);
  return (int)hipGetLastError();
}

int view_compose(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam, const unsigned* keys,
                 const unsigned* ids, const lemo_render_shade* sp, const unsigned* scene_key, const unsigned char* scene_rgb, const float* spheres,
                 int P, const float* radius, const unsigned char* sphere_rgb, int rgb_shared, const float* view, unsigned bg, unsigned char* rgb,
                 float* depth, int* owner, hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || !normals || !faces || !keys || !ids || !sp || !rgb || bg > 0xFFFFFFu) return LEMO_ERR_ARG;
  if ((scene_key == nullptr) != (scene_rgb == nullptr)) return LEMO_ERR_ARG;
  if (P < 0 || P > VW_MAXP) return LEMO_ERR_SHAPE;
  if (P > 0 && (!spheres || !radius || !sphere_rgb)) return LEMO_ERR_ARG;
  VwArgs a;
  for (int k = 0; k < 3; ++k) a.sh.base[k] = sp->base[k];
  a.sh.ambient = sp->ambient; a.sh.diffuse = sp->diffuse;
  for (float v : {a.sh.base[0], a.sh.base[1], a.sh.base[2], a.sh.ambient, a.sh.diffuse})
    if (!vw_unit_ok(v)) return LEMO_ERR_ARG;
  if (view)
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(view[k])) return LEMO_ERR_ARG;
  if (B < 1 || B > 65535 || V < 1 || F < 1 || F > (1 << 30) || (long long)B * V > (1ll << 30)) return LEMO_ERR_SHAPE;
  a.verts = verts; a.normals = normals; a.faces = faces; a.V = V; a.F = F; a.keys = keys; a.ids = ids;
  a.scene_key = scene_key; a.scene_rgb = scene_rgb; a.spheres = spheres; a.radius = radius; a.sphere_rgb = sphere_rgb;
  a.P = P; a.rgb_shared = rgb_shared ? 1 : 0;
  vw_xf(view, a.X);
  a.bg = (bg >> 16) | (bg & 0xFF00u) | ((bg & 0xFFu) << 16);
  a.rgb = rgb; a.depth = depth; a.owner = owner;
  a.p0 = (int)((uintptr_t)rgb & 3);
  // rows shift left by up to 3 pixels; with W a multiple of 4 every row shifts by the same amount
  const int shift = c.W % 4 == 0 ? (4 - a.p0) & 3 : VW_PPT - 1;
  const dim3 grid((c.W + shift + VW_TW - 1) / VW_TW, (c.H + VW_TH - 1) / VW_TH, B);
  hipLaunchKernelGGL(view_compose_kernel, grid, dim3(OC_BLOCK), 0, s, a, c);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
int lemo_view_transform(const float* points, long long n, const float* xf, float* out, void* stream) {
  return lemo::view_transform(points, n, xf, out, (hipStream_t)stream);
}
int lemo_view_scene_resolve(const float* verts, const float* normals, int V, const int* faces, int F, const lemo_occl_cam* cam, const unsigned* ids,
                            const unsigned char* colors, float ambient, float diffuse, int lit, unsigned char* rgb, void* stream) {
  return lemo::view_scene_resolve(verts, normals, V, faces, F, cam, ids, colors, ambient, diffuse, lit, rgb, (hipStream_t)stream);
}
int lemo_view_compose(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam,
                      const unsigned* keys, const unsigned* ids, const lemo_render_shade* shade_par, const unsigned* scene_key,
                      const unsigned char* scene_rgb, const float* spheres, int P, const float* radius, const unsigned char* sphere_rgb,
                      int rgb_shared, const float* view, unsigned bg, unsigned char* rgb, float* depth, int* owner, void* stream) {
  return lemo::view_compose(verts, normals, B, V, faces, F, cam, keys, ids, shade_par, scene_key, scene_rgb, spheres, P, radius, sphere_rgb,
                            rgb_shared, view, bg, rgb, depth, owner, (hipStream_t)stream);
}
}  // extern "C"
