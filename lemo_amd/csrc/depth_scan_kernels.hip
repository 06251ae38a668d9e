// Kinect depth frames to body scans, for B frames at once: the device form of the reference's Projection.create_scan
// (temp_prox/projection_utils.py:35-90) and of the per-frame truncate / pad / mean that follows it in the loader
// (temp_prox/data_parser_slide.py:283-323).  OpenCV is not part of this project's environment: cv2.undistortPoints and
// cv2.projectPoints are restated from OpenCV's documented model k = (k1, k2, p1, p2, k3), not confirmed by a run.
//
// Per pixel (ds_pixel, written once; every kernel below calls it).  Pixel i = v W + u of frame b, row-major:
//   depth   d = depth[b][v][u'] (float32 metres) or (raw[b][v][u'] / 8) depth_scale (uint16), u' = W - 1 - u with flip (:285-289);
//           with the depth-resolution mask (mask_on_color == 0), d = 0 where mask[b][v][u] != 0.  The caller's depth is not modified
//           (the reference overwrites it in place, projection_utils.py:56).  A depth that is not finite makes the pixel invalid.
//   ray     (x, y) = rays[v][u]: the undistorted normalised IR coordinate of the pixel, a constant of the calibration built on the
//           host in float64 (5 fixed-point iterations, cv2.undistortPoints' default) and rounded to fp32 once.
//   p       = ((x d, y d, d) - t_d) . R_d with view_mtx = [R_d | t_d] of the IR camera (:43-46): unproject_depth_image's result.
//   q       = R_c p + T_c (R_c from the Rodrigues vector, on the host in float64), pinhole division, radial + tangential distortion,
//           colour intrinsics -> (u_c, v_c), rounded with rintf (half to even, as np.round).
//   pc      = view_c . (p, 1) (coord == 'color') or p.
//   valid   mask_on_color: 0 <= u_c < cW, 0 <= v_c < cH, mask[b][v_c][u_c] == 0 and pc.z > TH;   else: pc.z > TH alone (the reference
//           does not apply the in-image test to the points in this branch, :78-81).
// fp32 VALU only.  Every product-sum is an explicit fmaf chain and contraction is off, so a pixel has ONE result whichever kernel
// evaluates it (pass A, pass C, lemo_depth_unproject) and on the host emulator: the compacted points are the per-pixel points, bit
// for bit.
//
// Ordered compaction without the return value of any atomic.  A workgroup is 256 threads = 4 waves and owns 256 consecutive pixels of
// one frame; grid (G = ceil(H W / 256), B).  The reference keeps the FIRST S surviving points in row-major order, so the order is part
// of the result.
//   pass A  ds_count_kernel: flags by ds_pixel, __ballot + popcount per wave, the four wave counts summed through LDS -> counts[b][g];
//           the group's sum of the valid pc in double (a butterfly over the wave, then wave 0 + 1 + 2 + 3: a fixed order) ->
//           psum[b][g][3].  On request also the per-pixel points [B][H][W][3] and flags [B][H][W].
//   pass B  ds_offsets_kernel, one workgroup per frame: exclusive scan of the frame's group counts, 256 at a time (wave scans by
//           __shfl_up, wave totals through LDS, a running carry) -> offsets[b][g], n_valid[b], scan_point_num[b] = min(n_valid, S);
//           the group sums added in group order by three lanes (x, y, z), divided by n_valid -> init_trans[b]: the mean over ALL
//           valid points, NaN for a frame without any (np.mean of an empty array).
//   pass C  ds_compact_kernel: ds_pixel again, rank = popcount of the ballot below the lane + the wave offsets through LDS; point
//           offset + rank goes to scan[b][offset + rank] while that is below S.  The same launch writes rows scan_point_num[b] .. S - 1
//           as zeros, so the output needs no initialisation.
// Memory-bound: pass A and C each read the depth (2 or 4 B), the ray (8 B) and, with mask_on_color, one gathered mask byte per pixel.
#include "geom_device.hpp"
#include "kernels.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace lemo {

#define DS_BLOCK 256
#define DS_WAVES (DS_BLOCK / 64)
#define DS_MAX_B 1024
#define DS_MAX_HW (1 << 22)
#define DS_MAX_S (1 << 20)

// the calibration and the options of one call, by value in the kernel arguments (scalar registers)
struct DsParams {
  float td[3], Rd[9], Rc[9], Tc[3], fx, fy, cx, cy, k[5], Vc[12];
  int cW, cH;
  float TH, depth_scale;
  int raw, flip, mask_on_color, coord_color;
};

struct DsPix { float p[3], pc[3]; bool valid; };

// depth of pixel (v, u) of the frame at `frame` (an element offset), before the depth-resolution mask
__device__ __forceinline__ float ds_depth(const void* __restrict__ depth, size_t frame, int W, int v, int u, const DsParams& P) {
  const size_t at = frame + (size_t)v * W + (P.flip ? W - 1 - u : u);
  if (P.raw) return ((float)static_cast<const unsigned short*>(depth)[at] * 0.125f) * P.depth_scale;
  return static_cast<const float*>(depth)[at];
}

// p = ((x d, y d, d) - t_d) . R_d
__device__ __forceinline__ void ds_unproject(float x, float y, float d, const DsParams& P, float p[3]) {
  const float c[3] = {fmaf(x, d, -P.td[0]), fmaf(y, d, -P.td[1]), d - P.td[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float col[3] = {P.Rd[j], P.Rd[3 + j], P.Rd[6 + j]};
    p[j] = dot3(c, col);
  }
}

// i: pixel of the frame (< H W); mask: this frame's mask (colour-sized or depth-sized, by the branch)
__device__ __forceinline__ void ds_pixel(const void* __restrict__ depth, size_t frame, const float* __restrict__ rays,
                                         const unsigned char* __restrict__ mask, int W, int i, const DsParams& P, DsPix& o) {
  const int v = i / W, u = i - v * W;
  float d = ds_depth(depth, frame, W, v, u, P);
  if (!P.mask_on_color && mask[i] != 0) d = 0.0f;
  const bool finite = fabsf(d) < INFINITY;                     // false for NaN as well
  const float x = rays[2 * (size_t)i], y = rays[2 * (size_t)i + 1];
  ds_unproject(x, y, d, P, o.p);
  if (P.coord_color) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.pc[j] = fmaf(P.Vc[4 * j + 2], o.p[2], fmaf(P.Vc[4 * j + 1], o.p[1], fmaf(P.Vc[4 * j], o.p[0], P.Vc[4 * j + 3])));
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.pc[j] = o.p[j];
  }
  bool ok = finite && o.pc[2] > P.TH;
  if (P.mask_on_color) {
    float q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = fmaf(P.Rc[3 * j + 2], o.p[2], fmaf(P.Rc[3 * j + 1], o.p[1], fmaf(P.Rc[3 * j], o.p[0], P.Tc[j])));
    const float xx = q[0] / q[2], yy = q[1] / q[2];
    const float r2 = fmaf(xx, xx, yy * yy);
    const float cd = fmaf(fmaf(fmaf(P.k[4], r2, P.k[1]), r2, P.k[0]), r2, 1.0f);
    const float a1 = 2.0f * xx * yy, a2 = fmaf(2.0f * xx, xx, r2), a3 = fmaf(2.0f * yy, yy, r2);
    const float xd = fmaf(xx, cd, fmaf(P.k[2], a1, P.k[3] * a2)), yd = fmaf(yy, cd, fmaf(P.k[2], a3, P.k[3] * a1));
    const float uc = rintf(fmaf(P.fx, xd, P.cx)), vc = rintf(fmaf(P.fy, yd, P.cy));
    const bool inside = uc >= 0.0f && uc <= (float)(P.cW - 1) && vc >= 0.0f && vc <= (float)(P.cH - 1);      // false for NaN
    ok = ok && inside && mask[(size_t)(inside ? (int)vc : 0) * P.cW + (inside ? (int)uc : 0)] == 0;
  }
  o.valid = ok;
}

__device__ __forceinline__ const unsigned char* ds_frame_mask(const unsigned char* __restrict__ mask, int b, int HW, const DsParams& P) {
  return mask + (size_t)b * (P.mask_on_color ? (size_t)P.cW * P.cH : (size_t)HW);
}

// ---- pass A ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DS_BLOCK) ds_count_kernel(const void* __restrict__ depth, const float* __restrict__ rays,
                                                            const unsigned char* __restrict__ mask, int H, int W, DsParams P, int G,
                                                            int* __restrict__ counts, double* __restrict__ psum, float* __restrict__ points,
                                                            unsigned char* __restrict__ valid) {
  __shared__ int s_cnt[DS_WAVES];
  __shared__ double s_sum[DS_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, b = blockIdx.y, HW = H * W;
  const int i = g * DS_BLOCK + tid;
  const bool in = i < HW;
  const size_t frame = (size_t)b * HW;
  DsPix px;
  ds_pixel(depth, frame, rays, ds_frame_mask(mask, b, HW, P), W, in ? i : HW - 1, P, px);      // the tail repeats the last pixel and stores nothing
  const bool ok = in && px.valid;
  if (in && points) {
    float* __restrict__ o = points + 3 * (frame + i);
    o[0] = px.pc[0]; o[1] = px.pc[1]; o[2] = px.pc[2];
    valid[frame + i] = ok ? 1 : 0;
  }
  const unsigned long long bal = __ballot(ok);
  double s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s[k] = ok ? (double)px.pc[k] : 0.0;
    for (int m = 32; m >= 1; m >>= 1) s[k] += __shfl_xor(s[k], m);
  }
  if (lane == 0) {
    s_cnt[wave] = __builtin_popcountll(bal);
    s_sum[wave][0] = s[0]; s_sum[wave][1] = s[1]; s_sum[wave][2] = s[2];
  }
  __syncthreads();
  if (tid == 0) counts[(size_t)b * G + g] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
  if (tid < 3) psum[3 * ((size_t)b * G + g) + tid] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DS_BLOCK) ds_offsets_kernel(const int* __restrict__ counts, const double* __restrict__ psum, int G, int S,
                                                              int* __restrict__ offsets, int* __restrict__ n_valid, int* __restrict__ scan_point_num,
                                                              float* __restrict__ init_trans) {
  __shared__ int s_tot[DS_WAVES];
  __shared__ double s_sum[3][DS_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int* __restrict__ c = counts + (size_t)b * G;
  const double* __restrict__ ps = psum + 3 * (size_t)b * G;
  int carry = 0;
  double acc = 0.0;                                            // lanes 0, 1, 2: x, y, z
  for (int g0 = 0; g0 < G; g0 += DS_BLOCK) {
    const int g = g0 + tid;
    const int n = g < G ? c[g] : 0;
    int x = n;                                                 // inclusive scan over the wave
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const int y = __shfl_up(x, dlt);
      if (lane >= dlt) x += y;
    }
    if (lane == 63) s_tot[wave] = x;
#pragma unroll
    for (int k = 0; k < 3; ++k) s_sum[k][tid] = g < G ? ps[3 * (size_t)g + k] : 0.0;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DS_WAVES; ++w) { before += w < wave ? s_tot[w] : 0; total += s_tot[w]; }
    if (g < G) offsets[(size_t)b * G + g] = carry + before + (x - n);
    carry += total;
    if (tid < 3) for (int j = 0; j < DS_BLOCK; ++j) acc += s_sum[tid][j];
    __syncthreads();
  }
  if (tid == 0) { n_valid[b] = carry; scan_point_num[b] = min(carry, S); }
  if (tid < 3) init_trans[3 * (size_t)b + tid] = (float)(acc / (double)carry);                // 0 / 0 = NaN: no valid point
}

// ---- pass C ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DS_BLOCK) ds_compact_kernel(const void* __restrict__ depth, const float* __restrict__ rays,
                                                              const unsigned char* __restrict__ mask, int H, int W, DsParams P, int G, int S,
                                                              const int* __restrict__ offsets, const int* __restrict__ scan_point_num,
                                                              float* __restrict__ scan) {
  __shared__ int s_cnt[DS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, b = blockIdx.y, HW = H * W;
  const int i = g * DS_BLOCK + tid;
  const bool in = i < HW;
  DsPix px;
  ds_pixel(depth, (size_t)b * HW, rays, ds_frame_mask(mask, b, HW, P), W, in ? i : HW - 1, P, px);
  const bool ok = in && px.valid;
  const unsigned long long bal = __ballot(ok);
  if (lane == 0) s_cnt[wave] = __builtin_popcountll(bal);
  __syncthreads();
  int at = offsets[(size_t)b * G + g] + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
#pragma unroll
  for (int w = 0; w < DS_WAVES; ++w) at += w < wave ? s_cnt[w] : 0;
  float* __restrict__ out = scan + 3 * (size_t)b * S;
  if (ok && at < S) {
    float* __restrict__ o = out + 3 * (size_t)at;
    o[0] = px.pc[0]; o[1] = px.pc[1]; o[2] = px.pc[2];
  }
  // the pad: floats 3 n .. 3 S - 1 of the frame, shared out over the frame's threads
  const long long lo = 3ll * scan_point_num[b], hi = 3ll * S, step = (long long)G * DS_BLOCK;
  for (long long r = lo + i; r < hi; r += step) out[r] = 0.0f;
}

// ---- per-pixel points alone ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DS_BLOCK) ds_unproject_kernel(const void* __restrict__ depth, const float* __restrict__ rays, int H, int W,
                                                                DsParams P, float* __restrict__ points) {
  const int HW = H * W, i = blockIdx.x * DS_BLOCK + threadIdx.x, b = blockIdx.y;
  if (i >= HW) return;
  const size_t frame = (size_t)b * HW;
  const int v = i / W, u = i - v * W;
  const float d = ds_depth(depth, frame, W, v, u, P);
  float p[3];
  ds_unproject(rays[2 * (size_t)i], rays[2 * (size_t)i + 1], d, P, p);
  float* __restrict__ o = points + 3 * (frame + i);
  o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

namespace {

int ds_shape(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || B > DS_MAX_B || (long long)H * W > DS_MAX_HW) return LEMO_ERR_SHAPE;
  return 0;
}

int ds_groups(int H, int W) { return (H * W + DS_BLOCK - 1) / DS_BLOCK; }

// 0, or why the calibration and the options are not taken
int ds_params(const lemo_depth_calib* cal, int raw, int flip, float depth_scale, int mask_on_color, int coord_color, float TH, bool project,
              DsParams& P) {
  if (!cal || !cal->rays) return LEMO_ERR_ARG;
  if (project && (cal->cW < 1 || cal->cH < 1 || cal->cW > 32768 || cal->cH > 32768)) return LEMO_ERR_SHAPE;
  if ((raw | flip | mask_on_color | coord_color) & ~1) return LEMO_ERR_ARG;
  if (!std::isfinite(depth_scale) || !std::isfinite(TH)) return LEMO_ERR_ARG;
  for (int r = 0; r < 3; ++r) {
    P.td[r] = cal->view_d[4 * r + 3];
    for (int c = 0; c < 3; ++c) P.Rd[3 * r + c] = cal->view_d[4 * r + c];
    P.Tc[r] = cal->Tc[r];
  }
  for (int k = 0; k < 9; ++k) P.Rc[k] = cal->Rc[k];
  for (int k = 0; k < 12; ++k) P.Vc[k] = cal->view_c[k];
  for (int k = 0; k < 5; ++k) P.k[k] = cal->k[k];
  P.fx = cal->fx; P.fy = cal->fy; P.cx = cal->cx; P.cy = cal->cy;
  P.cW = cal->cW; P.cH = cal->cH;
  P.TH = TH; P.depth_scale = depth_scale;
  P.raw = raw; P.flip = flip; P.mask_on_color = mask_on_color; P.coord_color = coord_color;
  return 0;
}

}  // namespace

long long depth_scan_ws_bytes(int B, int H, int W) {
  if (ds_shape(B, H, W)) return -1;
  return (long long)B * ds_groups(H, W) * (3 * (long long)sizeof(double) + 2 * (long long)sizeof(int));
}

int depth_scan(const void* depth, int raw, int flip, float depth_scale, const unsigned char* mask, int mask_on_color, int coord_color, float TH,
               const lemo_depth_calib* cal, int B, int H, int W, int S, float* scan, int* scan_point_num, int* n_valid, float* init_trans,
               float* points, unsigned char* valid, void* ws, long long ws_bytes, hipStream_t s) {
  if (int e = ds_shape(B, H, W)) return e;
  if (S < 1 || S > DS_MAX_S) return LEMO_ERR_SHAPE;
  DsParams P;
  if (int e = ds_params(cal, raw, flip, depth_scale, mask_on_color, coord_color, TH, true, P)) return e;
  if (!depth || !mask || !scan || !scan_point_num || !n_valid || !init_trans || (points == nullptr) != (valid == nullptr)) return LEMO_ERR_ARG;
  if (!ws || ws_bytes < depth_scan_ws_bytes(B, H, W)) return LEMO_ERR_ARG;
  const int G = ds_groups(H, W);
  double* psum = static_cast<double*>(ws);                      // [B][G][3], then counts [B][G], offsets [B][G]
  int* counts = reinterpret_cast<int*>(psum + 3 * (size_t)B * G);
  int* offsets = counts + (size_t)B * G;
  const dim3 blk(DS_BLOCK), grid(G, B);
  hipLaunchKernelGGL(ds_count_kernel, grid, blk, 0, s, depth, cal->rays, mask, H, W, P, G, counts, psum, points, valid);
  hipLaunchKernelGGL(ds_offsets_kernel, dim3(B), blk, 0, s, (const int*)counts, (const double*)psum, G, S, offsets, n_valid, scan_point_num,
                     init_trans);
  hipLaunchKernelGGL(ds_compact_kernel, grid, blk, 0, s, depth, cal->rays, mask, H, W, P, G, S, (const int*)offsets, (const int*)scan_point_num,
                     scan);
  return (int)hipGetLastError();
}

int depth_unproject(const void* depth, int raw, int flip, float depth_scale, const lemo_depth_calib* cal, int B, int H, int W, float* points,
                    hipStream_t s) {
  if (int e = ds_shape(B, H, W)) return e;
  DsParams P;
  if (int e = ds_params(cal, raw, flip, depth_scale, 0, 0, 0.0f, false, P)) return e;
  if (!depth || !points) return LEMO_ERR_ARG;
  hipLaunchKernelGGL(ds_unproject_kernel, dim3(ds_groups(H, W), B), dim3(DS_BLOCK), 0, s, depth, cal->rays, H, W, P, points);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
long long lemo_depth_scan_ws_bytes(int B, int H, int W) { return lemo::depth_scan_ws_bytes(B, H, W); }
int lemo_depth_scan(const void* depth, int raw, int flip, float depth_scale, const unsigned char* mask, int mask_on_color, int coord_color,
                    float TH, const lemo_depth_calib* cal, int B, int H, int W, int S, float* scan, int* scan_point_num, int* n_valid,
                    float* init_trans, float* points, unsigned char* valid, void* ws, long long ws_bytes, void* stream) {
  return lemo::depth_scan(depth, raw, flip, depth_scale, mask, mask_on_color, coord_color, TH, cal, B, H, W, S, scan, scan_point_num, n_valid,
                          init_trans, points, valid, ws, ws_bytes, (hipStream_t)stream);
}
int lemo_depth_unproject(const void* depth, int raw, int flip, float depth_scale, const lemo_depth_calib* cal, int B, int H, int W,
                         float* points, void* stream) {
  return lemo::depth_unproject(depth, raw, flip, depth_scale, cal, B, H, W, points, (hipStream_t)stream);
}
}  // extern "C"
