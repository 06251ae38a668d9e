// Body overlays on the device: what the render_results branch of the reference's temp_prox/fit_temp_loadprox_slide.py:622-683
// does with pyrender on the host -- the fitted body rendered in the PROX camera view, composited over the colour frame, the 2-D
// joints drawn on top -- as
//     vertex_normals_kernel     area-weighted vertex normals, a gather over the vertex -> face adjacency (CSR, built on the host
//                               once per topology): no float atomics, a fixed order of additions, the same bits in every run
//     render_walk_kernel<0>     the batched depth pass: the triangle-parallel walk of occlusion_kernels.hip (small boxes per thread,
//     render_walk_big_kernel<0>  big boxes per workgroup), the frame in blockIdx.y, atomicMax on keys [B][H][W]
//     render_walk_*<1>          the id pass, a launch of its own AFTER the depth pass: the same walk; where a face's key equals the
//                               pixel's winning key, atomicMax(ids, 0xFFFFFFFF - f) -> the lowest-index face among the nearest
//     render_resolve_kernel     per pixel: the id's face set up again, its edge functions at the pixel's ray -> perspective-correct
//                               weights -> interpolated normal -> head-light shade -> uint8; uncovered pixels copy the background
//     render_points_kernel      discs of one colour at pixel coordinates, over the body
// Coverage and depth are oc_setup / oc_key of raster_device.hpp, the functions lemo_depth_raster runs, so the depth of a rendered
// frame is bit for bit lemo_depth_raster's for that frame's mesh.  fp32 VALU with every operation spelled out (no contraction): the
// tests hold the kernels to a float32 numpy restatement operation by operation.
#include "raster_device.hpp"

#include <cstdint>

#pragma clang fp contract(off)

namespace lemo {

#define RN_PPT 4                                             // pixels per thread of the resolve: 12 bytes = 3 dwords of uint8 rgb

// ---- normals -----------------------------------------------------------------------------------------------------------------
// grid (vertex blocks, B)
__global__ void __launch_bounds__(OC_BLOCK) vertex_normals_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                  const int* __restrict__ adj_start, const int* __restrict__ adj_face, int nnz,
                                                                  float* __restrict__ normals, float* __restrict__ sums) {
  const int v = blockIdx.x * OC_BLOCK + threadIdx.x;
  if (v >= V) return;
  const float* vf = verts + (size_t)blockIdx.y * V * 3;
  const int lo = max(adj_start[v], 0), hi = min(adj_start[v + 1], nnz);      // a bad table cannot read outside adj_face
  float n[3] = {0.0f, 0.0f, 0.0f};
  for (int k = lo; k < hi; ++k) {
    const int f = adj_face[k];
    if ((unsigned)f >= (unsigned)F) continue;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const float *p0 = vf + 3 * (size_t)i0, *p1 = vf + 3 * (size_t)i1, *p2 = vf + 3 * (size_t)i2;
    float a[3], d2[3], c[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { a[q] = p1[q] - p0[q]; d2[q] = p2[q] - p0[q]; }
    oc_cross(a, d2, c);
#pragma unroll
    for (int q = 0; q < 3; ++q) n[q] = n[q] + c[q];
  }
  const size_t o = ((size_t)blockIdx.y * V + v) * 3;
  if (sums) { sums[o] = n[0]; sums[o + 1] = n[1]; sums[o + 2] = n[2]; }
  if (normals) {
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const bool ok = nn > 0.0f;
    const float len = sqrtf(nn);
    normals[o] = ok ? n[0] / len : 0.0f;
    normals[o + 1] = ok ? n[1] / len : 0.0f;
    normals[o + 2] = ok ? n[2] / len : 0.0f;
  }
}

// ---- depth pass (IDS = false) and id pass (IDS = true): one walk ------------------------------------------------------------
template <bool IDS>
__device__ __forceinline__ void rn_hit(unsigned k, int f, size_t i, unsigned* __restrict__ keys, unsigned* __restrict__ ids) {
  if (!k) return;
  if (!IDS) atomicMax(&keys[i], k);
  else if (k == keys[i]) atomicMax(&ids[i], 0xFFFFFFFFu - (unsigned)f);       // keys is final: the depth pass was an earlier launch
}

// grid (face blocks, B): one thread per triangle walks a bounding box of at most OC_BIG pixels
template <bool IDS>
__global__ void __launch_bounds__(OC_BLOCK) render_walk_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F, OcCam c,
                                                               unsigned* __restrict__ keys, unsigned* __restrict__ ids) {
  const int f = blockIdx.x * OC_BLOCK + threadIdx.x;
  OcXf X = {};
  OcTri t;
  if (f >= F || !oc_face(verts + (size_t)blockIdx.y * V * 3, V, faces, f, X, c, t) || oc_is_big(t)) return;
  const size_t base = (size_t)blockIdx.y * c.W * c.H;
  for (int y = t.y0; y <= t.y1; ++y) {
    const float dy = oc_ray_y(y, c);
    for (int x = t.x0; x <= t.x1; ++x) rn_hit<IDS>(oc_key(t, oc_ray_x(x, c), dy, c), f, base + (size_t)y * c.W + x, keys, ids);
  }
}

// the triangles above OC_BIG: every workgroup finds the big ones among its OC_BLOCK triangles, then strides one box at a time
template <bool IDS>
__global__ void __launch_bounds__(OC_BLOCK) render_walk_big_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                   OcCam c, unsigned* __restrict__ keys, unsigned* __restrict__ ids) {
  __shared__ int list[OC_BLOCK];
  __shared__ int count;
  const int tid = threadIdx.x, f = blockIdx.x * OC_BLOCK + tid;
  const float* vf = verts + (size_t)blockIdx.y * V * 3;
  const size_t base = (size_t)blockIdx.y * c.W * c.H;
  if (tid == 0) count = 0;
  __syncthreads();
  OcXf X = {};
  OcTri t;
  if (f < F && oc_face(vf, V, faces, f, X, c, t) && oc_is_big(t)) list[atomicAdd(&count, 1)] = f;
  __syncthreads();
  const int n = count;
  for (int i = 0; i < n; ++i) {
    const int fi = list[i];
    oc_face(vf, V, faces, fi, X, c, t);
    const int bw = t.x1 - t.x0 + 1, npix = bw * (t.y1 - t.y0 + 1);
    for (int q = tid; q < npix; q += OC_BLOCK) {
      const int y = t.y0 + q / bw, x = t.x0 + q % bw;
      rn_hit<IDS>(oc_key(t, oc_ray_x(x, c), oc_ray_y(y, c), c), fi, base + (size_t)y * c.W + x, keys, ids);
    }
  }
}

__global__ void __launch_bounds__(OC_BLOCK) render_depth_kernel(const unsigned* __restrict__ keys, float* __restrict__ depth, size_t n) {
  const size_t i = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i < n) depth[i] = oc_depth(keys[i]);
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------
// rn_quant and rn_shade (rule 3 of lemo_amd/render.py) live in raster_device.hpp: view_kernels.hip shades with the same functions
// One thread per group of RN_PPT pixels of the flat [B H W] pixel range.  Group g covers pixels p0 + 4 (g - 1) .. + 3 cut to [0, n):
// p0 = (address of rgb) mod 4 is the first pixel whose three bytes start on a dword, so every whole group is three aligned dwords
// whatever the image size and wherever in a larger tensor the frames start; group 0 (the p0 pixels before) and the last group go
// byte by byte.  The uint8 background is read the same way where its own address allows.
__global__ void __launch_bounds__(OC_BLOCK) render_resolve_kernel(const float* __restrict__ verts, const float* __restrict__ normals, int V,
                                                                  const int* __restrict__ faces, int F, OcCam c, const unsigned* __restrict__ ids, RnShade sh,
                                                                  const void* __restrict__ bg, int bg_kind, int bg_shared,
                                                                  unsigned char* __restrict__ rgb, int* __restrict__ face_ids,
                                                                  float* __restrict__ shade_out, size_t n, int p0) {
  const long long lo = (long long)p0 + RN_PPT * ((long long)((size_t)blockIdx.x * OC_BLOCK + threadIdx.x) - 1);
  if (lo >= (long long)n || lo + RN_PPT <= 0) return;
  const bool full = lo >= 0 && lo + RN_PPT <= (long long)n;
  const size_t HW = (size_t)c.W * c.H;
  const size_t first = lo < 0 ? 0 : (size_t)lo;
  unsigned b = (unsigned)(first / HW), pix = (unsigned)(first - (size_t)b * HW);
  unsigned id[RN_PPT], col[RN_PPT] = {0u, 0u, 0u, 0u};
  bool all = true;
#pragma unroll
  for (int j = 0; j < RN_PPT; ++j) {
    const long long p = lo + j;
    id[j] = (p >= 0 && p < (long long)n) ? ids[p] : 0u;
    if (0xFFFFFFFFu - id[j] >= (unsigned)F) id[j] = 0u;       // 0 = nothing hit; also an id that names no face
    all = all && id[j] != 0u;
  }
  if (bg_kind != LEMO_RENDER_BG_NONE && !all) {
    const size_t q0 = bg_shared ? (size_t)pix : first;         // the background's pixel of `first`
    const unsigned char* b8 = (const unsigned char*)bg;
    if (bg_kind == LEMO_RENDER_BG_U8 && full && (!bg_shared || (size_t)pix + RN_PPT <= HW) && (((uintptr_t)(b8 + 3 * q0)) & 3) == 0) {
      const unsigned* w = (const unsigned*)(b8 + 3 * q0);
      const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
      col[0] = w0 & 0xFFFFFFu;
      col[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
      col[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
      col[3] = w2 >> 8;
    } else {
      unsigned qp = pix;
      size_t qb = b;
#pragma unroll
      for (int j = 0; j < RN_PPT; ++j) {
        const long long p = lo + j;
        if (p < 0 || p >= (long long)n) continue;
        const size_t q = bg_shared ? (size_t)qp : qb * HW + qp;
        if (id[j] == 0u) {
          if (bg_kind == LEMO_RENDER_BG_U8) col[j] = b8[3 * q] | (b8[3 * q + 1] << 8) | (b8[3 * q + 2] << 16);
          else {
            const float* bf = (const float*)bg + 3 * q;
            col[j] = rn_quant(bf[0]) | (rn_quant(bf[1]) << 8) | (rn_quant(bf[2]) << 16);
          }
        }
        if (++qp == HW) { qp = 0; ++qb; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RN_PPT; ++j) {
    const long long p = lo + j;
    if (p < 0 || p >= (long long)n) continue;
    float shade = 0.0f;
    int fid = -1;
    if (id[j] != 0u) {
      fid = (int)(0xFFFFFFFFu - id[j]);
      const int y = (int)(pix / (unsigned)c.W), x = (int)(pix - (unsigned)y * (unsigned)c.W);
      shade = rn_shade(verts + (size_t)b * V * 3, normals + (size_t)b * V * 3, V, faces, fid, c, sh, x, y);
      col[j] = rn_quant(sh.base[0] * shade) | (rn_quant(sh.base[1] * shade) << 8) | (rn_quant(sh.base[2] * shade) << 16);
    }
    if (face_ids) face_ids[p] = fid;
    if (shade_out) shade_out[p] = shade;
    if (!full) { rgb[3 * p] = (unsigned char)col[j]; rgb[3 * p + 1] = (unsigned char)(col[j] >> 8); rgb[3 * p + 2] = (unsigned char)(col[j] >> 16); }
    if (++pix == HW) { pix = 0; ++b; }
  }
  if (full) {
    unsigned* w = (unsigned*)(rgb + 3 * (size_t)lo);
    w[0] = col[0] | (col[1] << 24);
    w[1] = (col[1] >> 8) | (col[2] << 16);
    w[2] = (col[2] >> 16) | (col[3] << 8);
  }
}

// ---- points: one thread per (frame, point, offset of the (2 r + 1)^2 square) -------------------------------------------------
__global__ void __launch_bounds__(OC_BLOCK) render_points_kernel(const float* __restrict__ pts, size_t total, int P, int r, int W, int H, unsigned color,
                                                                 unsigned char* __restrict__ rgb) {
  const size_t i = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int side = 2 * r + 1, per = side * side;
  const size_t q = i / per;
  const int o = (int)(i - q * per), dj = o / side - r, di = o % side - r;
  if (di * di + dj * dj > r * r) return;
  const float u = pts[2 * q], v = pts[2 * q + 1];
  if (!(fabsf(u) < 2147483520.0f && fabsf(v) < 2147483520.0f)) return;        // not finite, or no int
  const long long x = (long long)(int)u + di, y = (long long)(int)v + dj;     // truncation toward zero, as astype(int)
  if (x < 0 || x >= W || y < 0 || y >= H) return;
  unsigned char* d = rgb + (((q / P) * H + (size_t)y) * W + (size_t)x) * 3;
  d[0] = (unsigned char)(color >> 16); d[1] = (unsigned char)(color >> 8); d[2] = (unsigned char)color;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static int rn_mesh(int B, int V, int F) {
  if (B < 1 || B > 65535 || V < 1 || F < 1 || F > (1 << 30) || (long long)B * V > (1ll << 30)) return LEMO_ERR_SHAPE;
  return 0;
}

int vertex_normals(const float* verts, int B, int V, const int* faces, int F, const int* adj_start, const int* adj_face, int nnz,
                   float* normals, float* sums, hipStream_t s) {
  if (!verts || !faces || !adj_start || (!adj_face && nnz > 0) || (!normals && !sums)) return LEMO_ERR_ARG;
  if (int e = rn_mesh(B, V, F)) return e;
  if (nnz < 0) return LEMO_ERR_SHAPE;
  hipLaunchKernelGGL(vertex_normals_kernel, dim3((V + OC_BLOCK - 1) / OC_BLOCK, B), dim3(OC_BLOCK), 0, s, verts, V, faces, F, adj_start, adj_face,
                     nnz, normals, sums);
  return (int)hipGetLastError();
}

int render_ids(const float* verts, int B, int V, const int* faces, int F, const lemo_occl_cam* cam, unsigned* keys, unsigned* ids, float* depth,
               hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || !faces || !keys || !ids) return LEMO_ERR_ARG;
  if (int e = rn_mesh(B, V, F)) return e;
  const size_t n = (size_t)B * c.W * c.H;
  if (hipError_t e = hipMemsetAsync(keys, 0, n * sizeof(unsigned), s)) return (int)e;
  if (hipError_t e = hipMemsetAsync(ids, 0, n * sizeof(unsigned), s)) return (int)e;
  const dim3 grid((F + OC_BLOCK - 1) / OC_BLOCK, B), block(OC_BLOCK);
  hipLaunchKernelGGL(render_walk_kernel<false>, grid, block, 0, s, verts, V, faces, F, c, keys, ids);
  hipLaunchKernelGGL(render_walk_big_kernel<false>, grid, block, 0, s, verts, V, faces, F, c, keys, ids);
  hipLaunchKernelGGL(render_walk_kernel<true>, grid, block, 0, s, verts, V, faces, F, c, keys, ids);
  hipLaunchKernelGGL(render_walk_big_kernel<true>, grid, block, 0, s, verts, V, faces, F, c, keys, ids);
  if (depth) hipLaunchKernelGGL(render_depth_kernel, dim3((unsigned)((n + OC_BLOCK - 1) / OC_BLOCK)), block, 0, s, keys, depth, n);
  return (int)hipGetLastError();
}

int render_resolve(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam, const unsigned* ids,
                   const lemo_render_shade* sp, const void* background, int bg_kind, int bg_shared, unsigned char* rgb, int* face_ids,
                   float* shade, hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || !normals || !faces || !ids || !sp || !rgb) return LEMO_ERR_ARG;
  if (bg_kind != LEMO_RENDER_BG_NONE && bg_kind != LEMO_RENDER_BG_U8 && bg_kind != LEMO_RENDER_BG_F32) return LEMO_ERR_ARG;
  if (bg_kind != LEMO_RENDER_BG_NONE && !background) return LEMO_ERR_ARG;
  RnShade sh;
  for (int k = 0; k < 3; ++k) sh.base[k] = sp->base[k];
  sh.ambient = sp->ambient; sh.diffuse = sp->diffuse;
  for (float v : {sh.base[0], sh.base[1], sh.base[2], sh.ambient, sh.diffuse})
    if (!(v >= 0.f && v <= 1.f)) return LEMO_ERR_ARG;
  if (int e = rn_mesh(B, V, F)) return e;
  const size_t n = (size_t)B * c.W * c.H;
  const int p0 = (int)((uintptr_t)rgb & 3);
  const size_t groups = 1 + ((n > (size_t)p0 ? n - p0 : 0) + RN_PPT - 1) / RN_PPT;
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((groups + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s, verts, normals, V, faces, F,
                     c, ids, sh, background, bg_kind, bg_shared ? 1 : 0, rgb, face_ids, shade, n, p0);
  return (int)hipGetLastError();
}

int render_points(const float* points, int B, int P, int radius, int W, int H, unsigned color, unsigned char* rgb, hipStream_t s) {
  if (!points || !rgb || color > 0xFFFFFFu) return LEMO_ERR_ARG;
  if (B < 1 || B > 65535 || P < 1 || P > (1 << 20) || radius < 0 || radius > 16 || W < 1 || H < 1 || W > 32768 || H > 32768) return LEMO_ERR_SHAPE;
  const size_t side = 2 * (size_t)radius + 1, total = (size_t)B * P * side * side;
  if (total > ((size_t)1 << 38)) return LEMO_ERR_SHAPE;
  hipLaunchKernelGGL(render_points_kernel, dim3((unsigned)((total + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s, points, total, P, radius, W, H,
                     color, rgb);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
int lemo_vertex_normals(const float* verts, int B, int V, const int* faces, int F, const int* adj_start, const int* adj_face, int nnz,
                        float* normals, float* sums, void* stream) {
  return lemo::vertex_normals(verts, B, V, faces, F, adj_start, adj_face, nnz, normals, sums, (hipStream_t)stream);
}
int lemo_render_ids(const float* verts, int B, int V, const int* faces, int F, const lemo_occl_cam* cam, unsigned* keys, unsigned* ids,
                    float* depth, void* stream) {
  return lemo::render_ids(verts, B, V, faces, F, cam, keys, ids, depth, (hipStream_t)stream);
}
int lemo_render_resolve(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam,
                        const unsigned* ids, const lemo_render_shade* shade_par, const void* background, int bg_kind, int bg_shared,
                        unsigned char* rgb, int* face_ids, float* shade, void* stream) {
  return lemo::render_resolve(verts, normals, B, V, faces, F, cam, ids, shade_par, background, bg_kind, bg_shared, rgb, face_ids, shade,
                              (hipStream_t)stream);
}
int lemo_render_points(const float* points, int B, int P, int radius, int W, int H, unsigned color, unsigned char* rgb, void* stream) {
  return lemo::render_points(points, B, P, radius, W, H, color, rgb, (hipStream_t)stream);
}
}  // extern "C"
