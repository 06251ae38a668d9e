// Batch assembly for the two training engines: a step's batch gathered from a device-resident dataset, masked and reflect-padded
// exactly as the host recipes do it (lemo_amd/infill_train.py: network_tensors(mask_random_markers | mask_prox (clip_img), clip_img);
// lemo_amd/smooth_train.py: network_input), written straight into the engine's staging buffers.  Pure data movement: one thread
// per pixel of the padded H x W network image, lanes along the image's fastest axis (the frame), so a wave reads 64 consecutive
// frames of a row (mirrored in the 8 border columns) and the AE variant writes the four channels of a pixel as ONE 16-byte
// store.  No LDS, no atomics.
#include "train_epoch.hpp"

namespace lemo {

// torch's 'reflect' padding: the source index of padded index i of an n-long axis (pad < n: the entry points check it)
__device__ __forceinline__ int ep_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// an index the host wrapper has validated; the clamp only keeps a C caller's bad table from reading outside the dataset
__device__ __forceinline__ int ep_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

struct AePixel { float x0, x1, x2, x3, y; };

// THE index, mask and reflection arithmetic of the AE batch: pixel (r, w) of the H x W network image of batch slot c of `step`.
// d = H - 2 rows = 3 pelvis + 3 x 67 marker + 4 foot-contact rows when a recipe masks (the entry points check d == 208).
__device__ __forceinline__ AePixel aet_pixel(const EpochBlock& B, int step, int bs, int c, int r, int w, int H, int W) {
  const int d = H - 2, T = W - 16;
  const int sr = ep_reflect(r - 1, d), sc = ep_reflect(w - 8, T);
  const size_t slot = (size_t)step * bs + c;
  const int clip = ep_clamp(B.idx[slot], B.n_clips);
  const size_t ch = (size_t)d * T;
  const float* src = B.data + (size_t)clip * 4 * ch + (size_t)sr * T + sc;
  AePixel p{src[0], src[ch], src[2 * ch], src[3 * ch], 0.f};
  p.y = p.x0;
  const int marker = (sr >= 3 && sr < d - 4) ? (sr - 3) / 3 : -2;          // the marker whose 3 rows hold sr
  const int foot = sr >= d - 4 ? ((sr - (d - 4)) & 1) : -1;                // rows d-4, d-2: left (0); d-3, d-1: right (1)
  const int fa = foot ? 47 : 16, fb = foot ? 60 : 30;                      // the foot's two markers
  if (B.recipe == LEMO_MASK_RANDOM) {                                       // masked values are SET to 0
    const int* ids = B.marker_ids + slot * 6;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int id = ids[k];
      hit = hit || id == marker || (foot >= 0 && (id == fa || id == fb));
    }
    if (hit) p.x0 = 0.f;
  } else if (B.recipe == LEMO_MASK_PROX) {                                  // channel 0 is MULTIPLIED by the mask (the sign of a zero)
    const int L = B.mask_len;
    const float* m = B.masks + (size_t)ep_clamp(B.mask_idx[slot], B.n_masks) * 67 * L + sc;
    float mv = 1.f;                                                        // the pelvis rows
    if (marker >= 0) mv = m[(size_t)marker * L];
    else if (foot >= 0) mv = (m[(size_t)fa * L] == 1.f && m[(size_t)fb * L] == 1.f) ? 1.f : 0.f;
    p.x0 = p.x0 * mv;
  }
  return p;
}

// pixel (r, w) of the smoothness prior's network image: the velocity clip[..., 1:] - clip[..., :-1], a plain fp32 subtraction
__device__ __forceinline__ float sp_pixel(const EpochBlock& B, int step, int bs, int c, int r, int w, int H, int W) {
  const int d = H - 2, Tv = W - 16, T = Tv + 1;
  const int sr = ep_reflect(r - 1, d), sc = ep_reflect(w - 8, Tv);
  const int clip = ep_clamp(B.idx[(size_t)step * bs + c], B.n_clips);
  const float* src = B.data + ((size_t)clip * d + sr) * T + sc;
  return src[1] - src[0];
}

// API = false: the engine's layout (x: image c's CG8P x8 at x + c cs; y: ybuf); API = true: x [bs][4][H][W], y [bs][H][W].
// dev != null: the descriptor and the step come from device memory (the epoch's cursor), B and step are ignored.
template <bool API>
__global__ void __launch_bounds__(256)
aet_assemble_kernel(EpochBlock B, const EpochBlock* __restrict__ dev, int step, float* __restrict__ x, size_t cs, float* __restrict__ y,
                    int H, int W) {
  if (dev) { B = *dev; step = B.cursor; }
  const int p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, bs = gridDim.y, HW = H * W;
  if (p >= HW || step >= B.n_steps) return;
  const int r = p / W, w = p - r * W;
  const AePixel v = aet_pixel(B, step, bs, c, r, w, H, W);
  if (API) {
    float* o = x + (size_t)c * 4 * HW + p;
    o[0] = v.x0; o[HW] = v.x1; o[2 * (size_t)HW] = v.x2; o[3 * (size_t)HW] = v.x3;
  } else {
    st4(x + (size_t)c * cs + (size_t)((r + 1) * (W + 2) + w + 1) * 8, make_float4(v.x0, v.x1, v.x2, v.x3));
  }
  y[(size_t)c * HW + p] = v.y;
}

__global__ void __launch_bounds__(256)
sp_assemble_kernel(EpochBlock B, const EpochBlock* __restrict__ dev, int step, float* __restrict__ x, int H, int W) {
  if (dev) { B = *dev; step = B.cursor; }
  const int p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, bs = gridDim.y, HW = H * W;
  if (p >= HW || step >= B.n_steps) return;
  const int r = p / W, w = p - r * W;
  x[(size_t)c * HW + p] = sp_pixel(B, step, bs, c, r, w, H, W);
}

__global__ void __launch_bounds__(64)
ep_begin_kernel(EpochBlock B, EpochBlock* __restrict__ dev) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { B.cursor = 0; *dev = B; }
}

// the step's last kernel: one thread copies the losses into the log row of the step and advances the cursor
__global__ void __launch_bounds__(64)
ep_end_kernel(EpochBlock* __restrict__ dev, const float* __restrict__ losses, int nloss) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int s = dev->cursor;
  if (s >= dev->n_steps) return;
  float* row = dev->log + (size_t)s * nloss;
  for (int k = 0; k < nloss; ++k) row[k] = losses[k];
  dev->cursor = s + 1;
}

__global__ void __launch_bounds__(64)
train_step_counter_kernel(float* __restrict__ ctr, float* __restrict__ blob, int save) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int* ci = reinterpret_cast<int*>(ctr);
  if (save) {
    const int step = ci[0];
    blob[0] = (float)(step & 0xFFFFFF);
    blob[1] = (float)(step >> 24);
  } else {
    const int lo = (int)blob[0], hi = (int)blob[1];
    const int step = (lo & 0xFFFFFF) | ((hi & 0x7F) << 24);
    ci[0] = step;                                                // the bias corrections ctr[1], ctr[2] are rewritten by every step
  }
}

int ep_begin(const EpochBlock& B, EpochBlock* dev, hipStream_t s) {
  hipLaunchKernelGGL(ep_begin_kernel, dim3(1), dim3(64), 0, s, B, dev);
  return (int)hipGetLastError();
}
int ep_end(EpochBlock* dev, const float* losses, int nloss, hipStream_t s) {
  hipLaunchKernelGGL(ep_end_kernel, dim3(1), dim3(64), 0, s, dev, losses, nloss);
  return (int)hipGetLastError();
}
int aet_assemble(const EpochBlock& B, const EpochBlock* dev, int step, float* x8, size_t cs, float* ybuf, int bs, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL((aet_assemble_kernel<false>), dim3((H * W + 255) / 256, bs), dim3(256), 0, s, B, dev, step, x8, cs, ybuf, H, W);
  return (int)hipGetLastError();
}
int aet_assemble_api(const EpochBlock& B, int step, float* x, float* y, int bs, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL((aet_assemble_kernel<true>), dim3((H * W + 255) / 256, bs), dim3(256), 0, s, B, (const EpochBlock*)nullptr, step, x, (size_t)0, y, H, W);
  return (int)hipGetLastError();
}
int sp_assemble(const EpochBlock& B, const EpochBlock* dev, int step, float* x, int bs, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(sp_assemble_kernel, dim3((H * W + 255) / 256, bs), dim3(256), 0, s, B, dev, step, x, H, W);
  return (int)hipGetLastError();
}
int train_step_counter(float* ctr, float* blob, bool save, hipStream_t s) {
  hipLaunchKernelGGL(train_step_counter_kernel, dim3(1), dim3(64), 0, s, ctr, blob, save ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace lemo
