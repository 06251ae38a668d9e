// Device helpers shared by the mesh and point-cloud kernel families (visibility, depth_scan, selfpen, scene_sdf).  Each family
// promises the same bits in every mode; in part that rests on these being ONE function wherever they are used.
// Arithmetic: every function that rounds opens its body with `#pragma clang fp contract(off)` and spells its fused operations as fmaf,
// so it compiles to the same operations in every file that includes this header, whatever that file's own setting and wherever the
// #include stands.  Nothing here declares __shared__ storage: the kernels keep their arrays and pass them in.
#pragma once
#include <hip/hip_runtime.h>

namespace lemo {

#define GEOM_FMAX 3.0e38f                                    // a coordinate counts as finite iff |x| < GEOM_FMAX (false for NaN)

// ---- vector algebra: fp32, explicit fmaf ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot3(const float x[3], const float y[3]) {
#pragma clang fp contract(off)
  return fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0]));
}
__device__ __forceinline__ void cross3(const float x[3], const float y[3], float o[3]) {
#pragma clang fp contract(off)
  o[0] = fmaf(x[1], y[2], -(x[2] * y[1]));
  o[1] = fmaf(x[2], y[0], -(x[0] * y[2]));
  o[2] = fmaf(x[0], y[1], -(x[1] * y[0]));
}

// ---- grid primitives -----------------------------------------------------------------------------------------------------------------
// Two properties carry the exactness arguments of the grid searches:
//   float_key preserves order: x < y implies float_key(x) < float_key(y) for floats that are not NaN (and -0 sorts below +0), so the
//   largest key belongs to the largest value; float_unkey inverts it.
//   grid_cell is monotone non-decreasing in x for fixed (x0, sx) -- a subtraction, a product, a clamp, a truncation, each monotone in
//   fp32 -- and lies in [0, G - 1]; NaN gives cell 0.
__device__ __forceinline__ unsigned float_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ int grid_cell(float x, float x0, float sx, int G) {
#pragma clang fp contract(off)
  const float r = (x - x0) * sx;
  return (int)fminf(fmaxf(r, 0.0f), (float)(G - 1));
}

// ---- exclusive scan by one workgroup of BLOCK threads --------------------------------------------------------------------------------
// put(k, sum of get(0 .. k - 1)) for every k < n; returns the sum of all n to every thread.  Thread t owns the contiguous run
// [t per, (t + 1) per), per = ceil(n / BLOCK): a serial sum of its run, thread 0 over the BLOCK run totals in s_part, then the write-back.
// get(k) is read before put(k, .) is called, so put may overwrite what get reads (counters that become fill cursors).  A caller
// whose other threads then read what put wrote places a barrier behind the call.
template <int BLOCK, typename T, typename Get, typename Put>
__device__ __forceinline__ T block_exclusive_scan(int n, T* s_part, Get get, Put put) {
  const int tid = threadIdx.x;
  const int per = (n + BLOCK - 1) / BLOCK, lo = min(tid * per, n), hi = min(lo + per, n);
  T run = 0;
  for (int k = lo; k < hi; ++k) run += get(k);
  s_part[tid] = run;
  __syncthreads();
  if (tid == 0) {
    T acc = 0;
    for (int k = 0; k < BLOCK; ++k) { acc += s_part[k]; s_part[k] = acc; }      // inclusive: the last entry is the total
  }
  __syncthreads();
  T acc = tid ? s_part[tid - 1] : 0;
  for (int k = lo; k < hi; ++k) { const T v = get(k); put(k, acc); acc += v; }
  return s_part[BLOCK - 1];
}

// ---- face fetch ------------------------------------------------------------------------------------------------------------------------
// The index rule: face f is usable iff its three vertex indices lie in [0, V).  id holds the indices as stored: where the result is
// false nothing may be loaded through them (face_corners reads vertex 0 instead; a caller that loads by itself does the same), and what
// such a face then means is the caller's rule.
__device__ __forceinline__ bool face_ids(const int* __restrict__ faces, int f, int V, int id[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) { id[k] = faces[3 * (size_t)f + k]; ok = ok && (unsigned)id[k] < (unsigned)V; }
  return ok;
}
// The finite rule: the corners of the face with the indices id (from face_ids, with its result ok) -> ok and every coordinate finite.
// Once ok is false -- from the start for a bad index, behind a corner that is not finite -- the corners are read from vertex 0, which is
// in bounds: p is defined, and means nothing, when the result is false.
__device__ __forceinline__ bool face_corners(const float* __restrict__ vf, const int id[3], bool ok, float p[3][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = ok ? id[k] : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { p[k][a] = vf[3 * (size_t)i + a]; ok = ok && fabsf(p[k][a]) < GEOM_FMAX; }
  }
  return ok;
}

}  // namespace lemo
