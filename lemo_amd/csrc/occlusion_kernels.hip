// Occlusion masks of a PROX recording, on the device: what the reference's utils/get_occlusion_mask.py computes with two
// pyrender passes per frame,
//     :111-147   the static scene rendered once at 1920 x 1080 (IntrinsicsCamera, camera_pose = diag(1,-1,-1,1))  -> depth_scene
//     :170-184   the fitted SMPL-X body rendered per frame                                                        -> depth_body
//     :189-200   joints projected (fx = fy = 1060.53), truncated to pixels, occluded where the scene lies more than 0.1 m
//                in front of the body at that pixel
// as (a) a triangle-parallel depth raster for the scene and (b) a per-frame QUERY that evaluates the body's depth only at the
// P <= 128 pixels the mask reads, never the two million of the image.  Both call ONE pair of device functions (oc_setup, oc_key), so
// the body depth of the query is bit for bit the pixel a raster of the same mesh holds.
//
// Geometry.  Camera space is y down, z forward; pixel [y][x] samples the ray d = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1).
// Coverage uses homogeneous edge functions e_i = d . (p_j x (p_k - p_j)): the ray meets the triangle's plane inside the triangle
// iff the three have one sign.  They need no projected vertex, so a triangle that crosses the near plane or reaches behind the
// camera is handled per pixel without clipping.  Depth is the ray-plane intersection Z = (n . p0) / (n . d), n = (p1 - p0) x (p2 - p0);
// a hit counts iff znear <= Z <= zfar.  The nearest hit wins through atomicMax on the key 0xFFFFFFFF - float_bits(Z) (Z > 0: the bit
// patterns order like the values; 0 = no hit), which makes every image independent of the order of faces, threads and launches.
// fp32 VALU only, no fused multiply-adds the source does not spell out (the tests hold the kernels to a float32 numpy restatement
// operation by operation).
#include "raster_device.hpp"                                 // oc_setup, oc_key & co: shared with render_kernels.hip

#pragma clang fp contract(off)

namespace lemo {

// ---- (a) the raster: one thread per triangle walks a bounding box of at most OC_BIG pixels ----------------------------------
__global__ void __launch_bounds__(OC_BLOCK) depth_raster_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                OcXf X, OcCam c, unsigned* __restrict__ keys) {
  const int f = blockIdx.x * OC_BLOCK + threadIdx.x;
  OcTri t;
  if (f >= F || !oc_face(verts, V, faces, f, X, c, t) || oc_is_big(t)) return;
  for (int y = t.y0; y <= t.y1; ++y) {
    const float dy = oc_ray_y(y, c);
    for (int x = t.x0; x <= t.x1; ++x) {
      const unsigned k = oc_key(t, oc_ray_x(x, c), dy, c);
      if (k) atomicMax(&keys[(size_t)y * c.W + x], k);
    }
  }
}

// The few triangles above OC_BIG (walls, floor slabs, anything that crosses the near plane): every workgroup finds the big ones among
// its OC_BLOCK triangles, then strides the bounding box of one triangle at a time with all its threads.
__global__ void __launch_bounds__(OC_BLOCK) depth_raster_big_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                    OcXf X, OcCam c, unsigned* __restrict__ keys) {
  __shared__ int list[OC_BLOCK];
  __shared__ int count;
  const int tid = threadIdx.x, f = blockIdx.x * OC_BLOCK + tid;
  if (tid == 0) count = 0;
  __syncthreads();
  OcTri t;
  if (f < F && oc_face(verts, V, faces, f, X, c, t) && oc_is_big(t)) list[atomicAdd(&count, 1)] = f;
  __syncthreads();
  const int n = count;
  for (int i = 0; i < n; ++i) {
    oc_face(verts, V, faces, list[i], X, c, t);
    const int bw = t.x1 - t.x0 + 1, npix = bw * (t.y1 - t.y0 + 1);
    for (int q = tid; q < npix; q += OC_BLOCK) {
      const int y = t.y0 + q / bw, x = t.x0 + q % bw;
      const unsigned k = oc_key(t, oc_ray_x(x, c), oc_ray_y(y, c), c);
      if (k) atomicMax(&keys[(size_t)y * c.W + x], k);
    }
  }
}

__global__ void __launch_bounds__(OC_BLOCK) depth_resolve_kernel(unsigned* __restrict__ keys, size_t n) {
  const size_t i = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i < n) keys[i] = __float_as_uint(oc_depth(keys[i]));
}

// ---- (b) the query -----------------------------------------------------------------------------------------------------------
// PerspectiveCamera.forward (temp_prox/camera.py:113-115) then .astype(int) (:192): truncation toward zero, so u in (-1, 0) is
// column 0.  false: the projection is not finite or does not fit an int (such a point is visible; pix = OC_NOPIX).
__device__ __forceinline__ bool oc_project(const float* __restrict__ p, float pfx, float pfy, const OcCam& c, int& x, int& y) {
  const float u = pfx * (p[0] / p[2]) + c.cx, v = pfy * (p[1] / p[2]) + c.cy;
  x = OC_NOPIX; y = OC_NOPIX;
  if (!(fabsf(u) < 2147483520.0f && fabsf(v) < 2147483520.0f)) return false;
  x = (int)u; y = (int)v;
  return true;
}

// grid (face chunks, T).  keys [T][P], zeroed: nearest body key at each query pixel
__global__ void __launch_bounds__(OC_BLOCK) occlusion_query_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                   const float* __restrict__ pts, int P, OcCam c, float pfx, float pfy,
                                                                   unsigned* __restrict__ keys) {
  __shared__ float s_dx[OC_MAXP], s_dy[OC_MAXP];
  __shared__ int s_px[OC_MAXP], s_py[OC_MAXP];
  __shared__ unsigned s_key[OC_MAXP];
  __shared__ int s_box[4];
  const int tid = threadIdx.x, fr = blockIdx.y;
  if (tid < P) {
    int x, y;
    const bool ok = oc_project(pts + ((size_t)fr * P + tid) * 3, pfx, pfy, c, x, y) && x >= 0 && x < c.W && y >= 0 && y < c.H;
    s_px[tid] = ok ? x : OC_NOPIX;
    s_py[tid] = ok ? y : OC_NOPIX;
    s_dx[tid] = ok ? oc_ray_x(x, c) : 0.0f;
    s_dy[tid] = ok ? oc_ray_y(y, c) : 0.0f;
    s_key[tid] = 0u;
  }
  __syncthreads();
  if (tid == 0) {                                             // the box of the frame's pixels: most faces miss it altogether
    int x0 = c.W, x1 = -1, y0 = c.H, y1 = -1;
    for (int p = 0; p < P; ++p)
      if (s_px[p] != OC_NOPIX) { x0 = min(x0, s_px[p]); x1 = max(x1, s_px[p]); y0 = min(y0, s_py[p]); y1 = max(y1, s_py[p]); }
    s_box[0] = x0; s_box[1] = x1; s_box[2] = y0; s_box[3] = y1;
  }
  __syncthreads();
  const int bx0 = s_box[0], bx1 = s_box[1], by0 = s_box[2], by1 = s_box[3];
  if (bx1 < bx0) return;                                      // no point of this frame is in the image (the whole workgroup leaves)
  const float* vf = verts + (size_t)fr * V * 3;
  OcXf X;
  X.on = 0;
  for (int k = 0; k < OC_FPT; ++k) {
    const int f = (blockIdx.x * OC_FPT + k) * OC_BLOCK + tid;
    OcTri t;
    if (f >= F || !oc_face(vf, V, faces, f, X, c, t)) continue;
    if (t.x1 < bx0 || t.x0 > bx1 || t.y1 < by0 || t.y0 > by1) continue;
    for (int p = 0; p < P; ++p) {
      const int x = s_px[p], y = s_py[p];
      if (x < t.x0 || x > t.x1 || y < t.y0 || y > t.y1) continue;
      const unsigned key = oc_key(t, s_dx[p], s_dy[p], c);
      if (key) atomicMax(&s_key[p], key);
    }
  }
  __syncthreads();
  if (tid < P && s_key[tid]) atomicMax(&keys[(size_t)fr * P + tid], s_key[tid]);
}

// get_occlusion_mask.py:197-200 per (frame, point); 1 = visible
__global__ void __launch_bounds__(OC_BLOCK) occlusion_finish_kernel(const float* __restrict__ pts, int n, OcCam c, float pfx, float pfy,
                                                                    const unsigned* __restrict__ keys, const float* __restrict__ scene,
                                                                    float thresh, float* __restrict__ mask, float* __restrict__ depth_body,
                                                                    int* __restrict__ pix) {
  const int i = blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= n) return;
  int x, y;
  const bool in = oc_project(pts + (size_t)i * 3, pfx, pfy, c, x, y) && x >= 0 && x < c.W && y >= 0 && y < c.H;
  const float db = in ? oc_depth(keys[i]) : 0.0f;
  float m = 1.0f;
  if (in) {
    const float ds = scene[(size_t)y * c.W + x];
    if (ds != 0.0f && db - ds > thresh) m = 0.0f;
  }
  mask[i] = m;
  if (depth_body) depth_body[i] = db;
  if (pix) { pix[2 * (size_t)i] = x; pix[2 * (size_t)i + 1] = y; }
}

int depth_raster(const float* verts, int V, const int* faces, int F, const float* xf, const lemo_occl_cam* cam, float* depth, hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || !faces || !depth) return LEMO_ERR_ARG;
  if (V < 1 || F < 1 || F > (1 << 30)) return LEMO_ERR_SHAPE;
  OcXf X;
  X.on = xf != nullptr;
  for (int k = 0; k < 12; ++k) X.m[k] = xf ? xf[k] : 0.f;
  const size_t n = (size_t)c.W * c.H;
  unsigned* keys = reinterpret_cast<unsigned*>(depth);
  if (hipError_t e = hipMemsetAsync(keys, 0, n * sizeof(unsigned), s)) return (int)e;
  const dim3 grid((F + OC_BLOCK - 1) / OC_BLOCK);
  hipLaunchKernelGGL(depth_raster_kernel, grid, dim3(OC_BLOCK), 0, s, verts, V, faces, F, X, c, keys);
  hipLaunchKernelGGL(depth_raster_big_kernel, grid, dim3(OC_BLOCK), 0, s, verts, V, faces, F, X, c, keys);
  hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)((n + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s, keys, n);
  return (int)hipGetLastError();
}

int occlusion_query(const float* verts, int T, int V, const int* faces, int F, const float* points, int P, const lemo_occl_cam* cam,
                    float proj_fx, float proj_fy, const float* depth_scene, float thresh, unsigned* ws, float* mask, float* depth_body,
                    int* pix, hipStream_t s) {
  OcCam c;
  if (int e = oc_cam(cam, c)) return e;
  if (!verts || !faces || !points || !depth_scene || !ws || !mask) return LEMO_ERR_ARG;
  if (!(proj_fx > 0.f) || !(proj_fy > 0.f) || !std::isfinite(proj_fx) || !std::isfinite(proj_fy) || !std::isfinite(thresh)) return LEMO_ERR_ARG;
  if (P < 1 || P > OC_MAXP || T < 1 || T > 65535 || V < 1 || F < 1 || F > (1 << 30)) return LEMO_ERR_SHAPE;
  if (hipError_t e = hipMemsetAsync(ws, 0, (size_t)T * P * sizeof(unsigned), s)) return (int)e;
  const int per = OC_BLOCK * OC_FPT;
  hipLaunchKernelGGL(occlusion_query_kernel, dim3((F + per - 1) / per, T), dim3(OC_BLOCK), 0, s, verts, V, faces, F, points, P, c, proj_fx,
                     proj_fy, ws);
  const int n = T * P;
  hipLaunchKernelGGL(occlusion_finish_kernel, dim3((n + OC_BLOCK - 1) / OC_BLOCK), dim3(OC_BLOCK), 0, s, points, n, c, proj_fx, proj_fy, ws,
                     depth_scene, thresh, mask, depth_body, pix);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
int lemo_depth_raster(const float* verts, int V, const int* faces, int F, const float* xf, const lemo_occl_cam* cam, float* depth, void* stream) {
  return lemo::depth_raster(verts, V, faces, F, xf, cam, depth, (hipStream_t)stream);
}
int lemo_occlusion_query(const float* verts, int T, int V, const int* faces, int F, const float* points, int P, const lemo_occl_cam* cam,
                         float proj_fx, float proj_fy, const float* depth_scene, float thresh, unsigned* ws, float* mask,
                         float* depth_body, int* pix, void* stream) {
  return lemo::occlusion_query(verts, T, V, faces, F, points, P, cam, proj_fx, proj_fy, depth_scene, thresh, ws, mask, depth_body, pix,
                               (hipStream_t)stream);
}
}  // extern "C"
