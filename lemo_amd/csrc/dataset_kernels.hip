// Clip images of the two motion priors, built on the device from the SMPL-X markers of AMASS clips: what the reference's
// loaders do per clip on the host,
//     loader/train_loader_infill.py:134-277   mode local_markers_4chan -> [4][d][T-1], d = 3 (1 + M) + 4
//     loader/train_loader_smooth.py:130-176   mode local_markers       -> [1][d][T],   d = 3 (1 + M)
//     loader/train_loader_smooth.py:130-167   mode global_markers      -> [1][d][T],   d = 3 M  (what the shipped smoothness prior reads)
// followed by their dataset-wide statistics and normalisation (:281-330 / :180-204).  One workgroup per clip (T <= 256
// frames, like marker_kernels.hip).  The representation is computed by ONE device function, ds_value, after ds_prepare has
// left the clip's per-frame state in LDS; the statistics pass, the write pass and the [T][d] (API-layout) variant of the
// write pass all call it, so the numbers they see are the same.  Nothing of the dataset is kept in float64: the write pass
// recomputes the representation, normalises in float64 and rounds once to fp32.
//
// Precision follows the reference stage by stage: canonicalisation, contact labels and the floor shift in fp32 (torch
// float32 / numpy float32 there), everything from the reference joint on in float64 (numpy promotes at :223).
// Statistics: per-clip float64 partial sums (ds_stats_kernel), then one workgroup adds them in clip order
// (ds_stats_reduce_kernel) -- no float atomics, the result does not depend on how the clips were chunked into launches.
#include "kernels.hpp"

// No fused multiply-adds the source does not spell out: the fp32 stages reproduce torch / numpy float32 arithmetic operation by
// operation (the contact thresholds and the tests' float64 statistics bound depend on it), on the GPU as on the host emulator.
#pragma clang fp contract(off)

namespace lemo {

#define DS_T 256
#define DS_RADIUS 80                                         // gaussian_filter1d(sigma 20, truncate 4)
#define DS_KPAD 8                                            // scalar partials behind the d row sums

// per-clip state in LDS (10.3 KB)
struct ClipCtx {
  double a[DS_T], b[DS_T];                                   // forward direction (x, z); after the filter: root velocity (x, z)
  double g[DS_T];                                            // filter taps; after the filter: heading change
  double rc[DS_T], rs[DS_T];                                 // heading quaternion (w, y); then cos / sin of the heading angle
  float R[4];                                                // R0 = [x, z cross x, z]: (x_x, x_y, y_x, y_y)
  float org[3], morg[3];                                     // origin of the pelvis row / of the marker rows
  float floor_z, z_thr;
  float red[2 * DS_T / 64];
  unsigned char lbl[DS_T];                                   // 4 contact bits per frame
};

__host__ __device__ __forceinline__ int ds_rows_of(int M, int mode) {
  return mode == LEMO_CLIP_GLOBAL ? 3 * M : 3 * (M + 1) + (mode == LEMO_CLIP_4CHAN ? 4 : 0);
}
__device__ __forceinline__ int ds_rows(const lemo_clip_repr_desc& D) { return ds_rows_of(D.M, D.mode); }
// body slots of three rows each: pelvis + markers, or (global_markers) the markers alone
__device__ __forceinline__ int ds_slots(const lemo_clip_repr_desc& D) { return D.mode == LEMO_CLIP_GLOBAL ? D.M : D.M + 1; }
__device__ __forceinline__ int ds_frames(const lemo_clip_repr_desc& D) { return D.mode == LEMO_CLIP_4CHAN ? D.T - 1 : D.T; }

// (p - org) . R0 in fp32; the up column of R0 is (0, 0, 1)
__device__ __forceinline__ void ds_canon(const ClipCtx& c, const float* __restrict__ p, const float* org, float& x, float& y, float& z) {
  const float dx = p[0] - org[0], dy = p[1] - org[1];
  z = p[2] - org[2];
  x = fmaf(dy, c.R[1], dx * c.R[0]);
  y = fmaf(dy, c.R[3], dx * c.R[2]);
}
__device__ __forceinline__ const float* ds_marker(const lemo_clip_repr_desc& D, int n, int t, int m) {
  return D.markers + (((size_t)n * D.T + t) * D.M + m) * 3;
}
__device__ __forceinline__ const float* ds_pelvis(const lemo_clip_repr_desc& D, int n, int t) {
  return D.pelvis + ((size_t)n * D.T + t) * 3;
}

// Everything of clip n that is per clip or per frame; all DS_T threads call.
__device__ void ds_prepare(const lemo_clip_repr_desc& D, int n, ClipCtx& c) {
  const int t = threadIdx.x, T = D.T, M = D.M;
  if (t == 0) {
    // first-frame canonicalisation (train_loader_infill.py:136-143): x axis from the hips, up component zeroed
    const float* h = D.hips0 + (size_t)n * 6;
    float xx = h[3] - h[0], xy = h[4] - h[1];
    const float nx = sqrtf(xx * xx + xy * xy);
    xx /= nx; xy /= nx;
    float yx = -xy, yy = xx;                                  // z cross x
    const float ny = sqrtf(yx * yx + yy * yy);
    yx /= ny; yy /= ny;
    c.R[0] = xx; c.R[1] = xy; c.R[2] = yx; c.R[3] = yy;
    const float* p0 = ds_pelvis(D, n, 0);
    const float* m0 = D.mode == LEMO_CLIP_4CHAN ? p0 : ds_marker(D, n, 0, 0);      // train_loader_smooth.py:142-143
    for (int k = 0; k < 3; ++k) { c.org[k] = p0[k]; c.morg[k] = m0[k]; }
  }
  __syncthreads();
  if (D.mode != LEMO_CLIP_4CHAN) return;
  // ---- lowest marker (contact threshold, :192) and lowest row of pelvis + markers ("put on floor", :220)
  float mn = 3.4e38f, mnp = 3.4e38f;
  for (int w = t; w < T * M; w += DS_T) mn = fminf(mn, D.markers[((size_t)n * T * M + w) * 3 + 2] - c.org[2]);
  if (t < T) mnp = ds_pelvis(D, n, t)[2] - c.org[2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mnp = fminf(mnp, __shfl_xor(mnp, o)); }
  if ((t & 63) == 0) { c.red[t >> 6] = mn; c.red[DS_T / 64 + (t >> 6)] = mnp; }
  if (t <= 2 * DS_RADIUS) { const int k = t - DS_RADIUS; c.g[t] = exp(-0.5 * (double)(k * k) / 400.0); }
  __syncthreads();
  if (t == 0) {
    float m = c.red[0], mp = c.red[DS_T / 64];
    for (int i = 1; i < DS_T / 64; ++i) { m = fminf(m, c.red[i]); mp = fminf(mp, c.red[DS_T / 64 + i]); }
    c.z_thr = m + 0.10f;
    c.floor_z = fminf(m, mp);
  }
  __syncthreads();
  if (t < T) {
    // ---- forward direction (:238-244): across = (sdr_r - sdr_l) + (hip_r - hip_l) of the local, floor-shifted body
    float px, py, pz;
    ds_canon(c, ds_pelvis(D, n, t), c.org, px, py, pz);
    double q[4][3];
    const int ids[4] = {26, 56, 27, 57};                     // sdr_l, sdr_r, hip_l, hip_r
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x, y, z;
      ds_canon(c, ds_marker(D, n, t, ids[k]), c.morg, x, y, z);
      q[k][0] = (double)x - (double)px; q[k][1] = (double)y - (double)py; q[k][2] = (double)(z - c.floor_z);
    }
    const double ax = (q[1][0] - q[0][0]) + (q[3][0] - q[2][0]), ay = (q[1][1] - q[0][1]) + (q[3][1] - q[2][1]),
                 au = (q[1][2] - q[0][2]) + (q[3][2] - q[2][2]);
    const double nrm = sqrt(ax * ax + au * au + ay * ay);
    c.a[t] = -(ay / nrm); c.b[t] = ax / nrm;                  // across x up
    // ---- contact labels (:178-199): slow AND low; the last frame has no speed, it is low only
    const int foot[4] = {16, 47, 30, 60};
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x0, y0, z0;
      ds_canon(c, ds_marker(D, n, t, foot[k]), c.morg, x0, y0, z0);
      bool on = z0 < c.z_thr;
      if (t < T - 1) {
        float x1, y1, z1;
        ds_canon(c, ds_marker(D, n, t + 1, foot[k]), c.morg, x1, y1, z1);
        const float vx = (x1 - x0) * D.fps, vy = (y1 - y0) * D.fps, vz = (z1 - z0) * D.fps;
        on = on && sqrtf(vx * vx + vy * vy + vz * vz) < 0.22f;
      }
      bits |= on ? 1u << k : 0u;
    }
    c.lbl[t] = (unsigned char)bits;
  }
  __syncthreads();
  // ---- gaussian_filter1d over time, mode 'nearest' (:245), then Quaternions.between(forward, (0,0,1)) (:250)
  double qw = 1.0, qy = 0.0;
  if (t < T) {
    double wsum = 0.0, gx = 0.0, gz = 0.0;
    for (int k = 0; k <= 2 * DS_RADIUS; ++k) wsum += c.g[k];
    for (int k = 0; k <= 2 * DS_RADIUS; ++k) {
      int i = t + k - DS_RADIUS; i = i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
      const double w = c.g[k] / wsum;
      gx += w * c.a[i]; gz += w * c.b[i];
    }
    const double nrm = sqrt(gx * gx + gz * gz);
    gx /= nrm; gz /= nrm;
    const double w = sqrt(gx * gx + gz * gz) + gz, y = -gx;
    const double qn = sqrt(w * w + y * y);
    qw = w / qn; qy = y / qn;
    c.rc[t] = qw; c.rs[t] = qy;
  }
  __syncthreads();
  // ---- root velocity in the next frame's heading and the heading change (:254-255)
  double gvx = 0.0, gvy = 0.0, gr = 0.0;
  if (t < T - 1) {
    float x0, y0, z0, x1, y1, z1;
    ds_canon(c, ds_pelvis(D, n, t), c.org, x0, y0, z0);
    ds_canon(c, ds_pelvis(D, n, t + 1), c.org, x1, y1, z1);
    const double vx = (double)x1 - (double)x0, vy = (double)y1 - (double)y0;
    const double w1 = c.rc[t + 1], y1q = c.rs[t + 1];
    const double cs = w1 * w1 - y1q * y1q, sn = 2.0 * w1 * y1q;
    gvx = cs * vx + sn * vy; gvy = -sn * vx + cs * vy;
    const double pw = w1 * qw + y1q * qy, py = y1q * qw - w1 * qy;
    gr = atan2(2.0 * pw * py, pw * pw - py * py);
  }
  if (t == 0 && D.rot_0_pivot) D.rot_0_pivot[n] = atan2(2.0 * qw * qy, qw * qw - qy * qy);
  __syncthreads();
  if (t < T) {
    c.a[t] = gvx; c.b[t] = gvy; c.g[t] = gr;
    c.rc[t] = qw * qw - qy * qy; c.rs[t] = 2.0 * qw * qy;
  }
  __syncthreads();
}

// The three rows of body slot j (0 = pelvis, 1 + m = marker m; global_markers: j = marker j, no pelvis) at frame i, unnormalised.
__device__ __forceinline__ void ds_body(const lemo_clip_repr_desc& D, int n, const ClipCtx& c, int j, int i, double v[3]) {
  float px, py, pz, x, y, z;
  if (D.mode == LEMO_CLIP_GLOBAL) {                          // (p - marker 0 of frame 0) . R0, fp32 (train_loader_smooth.py:143, 165)
    ds_canon(c, ds_marker(D, n, i, j), c.morg, x, y, z);
    v[0] = x; v[1] = y; v[2] = z;
    return;
  }
  ds_canon(c, ds_pelvis(D, n, i), c.org, px, py, pz);
  if (j == 0) { x = px; y = py; z = pz; }
  else ds_canon(c, ds_marker(D, n, i, j - 1), c.morg, x, y, z);
  if (D.mode == LEMO_CLIP_4CHAN) {
    const double lx = (double)x - (double)px, ly = (double)y - (double)py;
    v[0] = c.rc[i] * lx + c.rs[i] * ly;
    v[1] = -c.rs[i] * lx + c.rc[i] * ly;
    v[2] = (double)(z - c.floor_z);
  } else if (j == 0) {
    v[0] = px; v[1] = py; v[2] = pz;
  } else {                                                   // markers relative to the pelvis, fp32 (train_loader_smooth.py:172)
    v[0] = (double)(x - px); v[1] = (double)(y - py); v[2] = (double)(z - pz);
  }
}

// THE representation: channel ch, row r, frame i of clip n, unnormalised, float64.
__device__ __forceinline__ double ds_value(const lemo_clip_repr_desc& D, int n, const ClipCtx& c, int ch, int r, int i) {
  if (ch == 1) return c.a[i];
  if (ch == 2) return c.b[i];
  if (ch == 3) return c.g[i];
  const int nb = 3 * ds_slots(D);
  if (r >= nb) return (double)((c.lbl[i] >> (r - nb)) & 1);
  double v[3];
  ds_body(D, n, c, r / 3, i, v);
  return v[r % 3];
}

// stats [2 d + 4]: mean[d], std[d], then (4chan) mean / std of channels 1-2 and of channel 3.  local_markers normalises
// rows 0-2 only (train_loader_smooth.py:200), global_markers every row (:191).
__device__ __forceinline__ float ds_norm(const lemo_clip_repr_desc& D, int d, int ch, int r, double v) {
  const double* s = D.stats;
  if (!s) return (float)v;
  if (ch == 0) return (D.mode != LEMO_CLIP_SMOOTH || r < 3) ? (float)((v - s[r]) / s[d + r]) : (float)v;
  return ch < 3 ? (float)((v - s[2 * d]) / s[2 * d + 1]) : (float)((v - s[2 * d + 2]) / s[2 * d + 3]);
}

// partials of clip n: part[r < d] = sum over frames of row r of channel 0, then
//   [d + 0] sum of squares of channel 0     [d + 1] ... of its rows 0-2 (global_markers: the sum of channel 0)
//   [d + 2], [d + 3] sum, sum of squares of channels 1-2     [d + 4], [d + 5] of channel 3
__global__ void __launch_bounds__(DS_T) ds_stats_kernel(lemo_clip_repr_desc D) {
  __shared__ ClipCtx c;
  const int n = blockIdx.x, t = threadIdx.x, d = ds_rows(D), F = ds_frames(D);
  ds_prepare(D, n, c);
  double* part = D.stats_part + (size_t)n * (d + DS_KPAD);
  double s = 0.0, ss = 0.0;
  if (t < d)
    for (int i = 0; i < F; ++i) { const double v = ds_value(D, n, c, 0, t, i); s += v; ss += v * v; }
  double g[4] = {0.0, 0.0, 0.0, 0.0};
  if (t == 0 && D.mode == LEMO_CLIP_4CHAN)
    for (int i = 0; i < F; ++i) {
      g[0] += c.a[i]; g[1] += c.a[i] * c.a[i];
      g[0] += c.b[i]; g[1] += c.b[i] * c.b[i];
      g[2] += c.g[i]; g[3] += c.g[i] * c.g[i];
    }
  __syncthreads();
  if (t < d) { part[t] = s; c.a[t] = ss; c.b[t] = s; }
  __syncthreads();
  if (t == 0) {
    double all = 0.0, head = 0.0;
    for (int r = 0; r < d; ++r) { all += c.a[r]; if (r == 2) head = all; }
    if (D.mode == LEMO_CLIP_GLOBAL) {
      head = 0.0;
      for (int r = 0; r < d; ++r) head += c.b[r];
    }
    part[d] = all; part[d + 1] = head;
    for (int k = 0; k < 4; ++k) part[d + 2 + k] = g[k];
    part[d + 6] = 0.0; part[d + 7] = 0.0;
  }
}

__global__ void __launch_bounds__(DS_T) ds_stats_reduce_kernel(const double* __restrict__ part, int N, int T, int M, int mode, double* __restrict__ stats) {
  __shared__ double tot[DS_T + DS_KPAD];
  const int t = threadIdx.x, d = ds_rows_of(M, mode), K = d + DS_KPAD;
  for (int k = t; k < K; k += DS_T) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += part[(size_t)n * K + k];       // clip order: independent of the launches that wrote them
    tot[k] = s;
  }
  __syncthreads();
  const double cnt = (double)N * (double)(mode == LEMO_CLIP_4CHAN ? T - 1 : T);
  double sum = 0.0, head = 0.0;
  for (int r = 0; r < d; ++r) { sum += tot[r]; if (r == 2) head = sum; }
  const double m_all = sum / (cnt * d), sd_all = sqrt(fmax(0.0, tot[d] / (cnt * d) - m_all * m_all));      // fmax: rounding must not make a variance negative
  const double m_head = head / (cnt * 3), sd_head = sqrt(fmax(0.0, tot[d + 1] / (cnt * 3) - m_head * m_head));
  if (mode == LEMO_CLIP_GLOBAL) {                            // one scalar std of the whole array, broadcast (train_loader_smooth.py:185)
    const double m_tot = tot[d + 1] / (cnt * d), sd_tot = sqrt(fmax(0.0, tot[d] / (cnt * d) - m_tot * m_tot));
    if (t < d) { stats[t] = tot[t] / cnt; stats[d + t] = sd_tot; }
    if (t == 0) { stats[2 * d] = sd_tot; stats[2 * d + 1] = sd_tot; stats[2 * d + 2] = 0.0; stats[2 * d + 3] = 0.0; }
  } else if (mode == LEMO_CLIP_4CHAN) {
    if (t < d) { stats[t] = t < d - 4 ? tot[t] / cnt : 0.0; stats[d + t] = t < d - 4 ? sd_all : 1.0; }
    if (t == 0) {
      const double mxy = tot[d + 2] / (2 * cnt), mr = tot[d + 4] / cnt;
      stats[2 * d] = mxy; stats[2 * d + 1] = sqrt(fmax(0.0, tot[d + 3] / (2 * cnt) - mxy * mxy));
      stats[2 * d + 2] = mr; stats[2 * d + 3] = sqrt(fmax(0.0, tot[d + 5] / cnt - mr * mr));
    }
  } else {
    if (t < d) { stats[t] = tot[t] / cnt; stats[d + t] = t < 3 ? sd_head : sd_all; }
    if (t == 0) { stats[2 * d] = sd_all; stats[2 * d + 1] = sd_head; stats[2 * d + 2] = 0.0; stats[2 * d + 3] = 0.0; }
  }
}

// API = false: the trainers' layout [N][C][d][F], lanes along the frame axis (a wave stores 64 consecutive floats);
// API = true: [N][C][F][d] as markers.get_local_markers_4chan returns it, lanes along the rows.
template <bool API>
__global__ void __launch_bounds__(DS_T) ds_write_kernel(lemo_clip_repr_desc D) {
  __shared__ ClipCtx c;
  __shared__ float vn[3][DS_T];
  const int n = blockIdx.x, t = threadIdx.x, d = ds_rows(D), F = ds_frames(D), M = D.M;
  const int wave = t >> 6, lane = t & 63, NW = DS_T / 64, nslot = ds_slots(D);
  const bool four = D.mode == LEMO_CLIP_4CHAN;
  ds_prepare(D, n, c);
  float* img = D.image + (size_t)n * (four ? 4 : 1) * d * F;
  if (four) {
    if (t < F)
      for (int ch = 1; ch < 4; ++ch) vn[ch - 1][t] = ds_norm(D, d, ch, 0, ds_value(D, n, c, ch, 0, t));
    if (D.contact && t < D.T)
      for (int k = 0; k < 4; ++k) D.contact[((size_t)n * D.T + t) * 4 + k] = (float)((c.lbl[t] >> k) & 1);
    __syncthreads();
  }
  if (API) {
    for (int i = wave; i < F; i += NW)
      for (int r = lane; r < d; r += 64) {
        img[(size_t)i * d + r] = ds_norm(D, d, 0, r, ds_value(D, n, c, 0, r, i));
        if (four)
          for (int ch = 1; ch < 4; ++ch) img[((size_t)ch * F + i) * d + r] = vn[ch - 1][i];
      }
    return;
  }
  for (int j = wave; j < nslot; j += NW)
    for (int i = lane; i < F; i += 64) {
      double v[3];
      ds_body(D, n, c, j, i, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) img[(size_t)(3 * j + k) * F + i] = ds_norm(D, d, 0, 3 * j + k, v[k]);
    }
  if (!four) return;
  for (int r = 3 * (M + 1) + wave; r < d; r += NW)
    for (int i = lane; i < F; i += 64) img[(size_t)r * F + i] = ds_norm(D, d, 0, r, ds_value(D, n, c, 0, r, i));
  // channels 1-3 are one value per frame, repeated over the d rows: every wave stores whole rows
  for (int w = wave; w < 3 * d; w += NW) {
    const int ch = w / d, r = w - ch * d;
    for (int i = lane; i < F; i += 64) img[((size_t)(1 + ch) * d + r) * F + i] = vn[ch][i];
  }
}

static int ds_check_shape(int n_clips, int T, int M, int mode) {
  // foot markers 16 / 47 / 30 / 60 and direction markers 26 / 27 / 56 / 57; the statistics pass runs one thread per row
  if (n_clips < 1 || T < 2 || T > DS_T || M < 61 || 3 * (M + 1) + 4 > DS_T) return LEMO_ERR_SHAPE;
  if (mode == LEMO_CLIP_GLOBAL && M != 67 && M != 81) return LEMO_ERR_SHAPE;      // the two marker sets of the smoothness loader
  return 0;
}

static int ds_check(const lemo_clip_repr_desc* D) {
  if (!D || !D->markers || !D->pelvis || !D->hips0) return LEMO_ERR_ARG;
  if (D->mode < LEMO_CLIP_4CHAN || D->mode > LEMO_CLIP_GLOBAL) return LEMO_ERR_ARG;
  return ds_check_shape(D->n_clips, D->T, D->M, D->mode);
}

int clip_repr_stats(const lemo_clip_repr_desc* D, hipStream_t s) {
  if (int e = ds_check(D)) return e;
  if (!D->stats_part) return LEMO_ERR_ARG;
  hipLaunchKernelGGL(ds_stats_kernel, dim3(D->n_clips), dim3(DS_T), 0, s, *D);
  return (int)hipGetLastError();
}

int clip_repr_stats_reduce(const double* part, int n_clips, int T, int M, int mode, double* stats, hipStream_t s) {
  if (!part || !stats || mode < LEMO_CLIP_4CHAN || mode > LEMO_CLIP_GLOBAL) return LEMO_ERR_ARG;
  if (int e = ds_check_shape(n_clips, T, M, mode)) return e;
  hipLaunchKernelGGL(ds_stats_reduce_kernel, dim3(1), dim3(DS_T), 0, s, part, n_clips, T, M, mode, stats);
  return (int)hipGetLastError();
}

int clip_repr_write(const lemo_clip_repr_desc* D, hipStream_t s) {
  if (int e = ds_check(D)) return e;
  if (!D->image) return LEMO_ERR_ARG;
  if (D->api_layout) hipLaunchKernelGGL((ds_write_kernel<true>), dim3(D->n_clips), dim3(DS_T), 0, s, *D);
  else hipLaunchKernelGGL((ds_write_kernel<false>), dim3(D->n_clips), dim3(DS_T), 0, s, *D);
  return (int)hipGetLastError();
}

}  // namespace lemo

extern "C" {
int lemo_clip_repr_stats_k(int M, int mode) { return lemo::ds_rows_of(M, mode) + DS_KPAD; }
int lemo_clip_repr_stats(const lemo_clip_repr_desc* d, void* stream) { return lemo::clip_repr_stats(d, (hipStream_t)stream); }
int lemo_clip_repr_stats_reduce(const double* stats_part, int n_clips, int T, int M, int mode, double* stats, void* stream) {
  return lemo::clip_repr_stats_reduce(stats_part, n_clips, T, M, mode, stats, (hipStream_t)stream);
}
int lemo_clip_repr_write(const lemo_clip_repr_desc* d, void* stream) { return lemo::clip_repr_write(d, (hipStream_t)stream); }
}  // extern "C"
