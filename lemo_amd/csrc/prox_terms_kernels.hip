// Optional terms of the PROX window engine (lemo_prox_set_terms): what SMPLifyLoss.forward adds with `contact`, `s2m` / `m2s`,
// `interpenetration` and `smooth_acc` / `smooth_vel` switched on (fitting_temp_slide.py:743-753, :637-670, :618-635, :756-772), as the
// finish and adjoint kernels around the searches the engine reuses (lemo_chamfer_forward / _masked_forward, lemo_vertex_visibility,
// lemo_selfpen_search / _loss_forward).  lemo_amd/prox.py's ProxTemporalFitter.loss_dict states the same terms in torch.
//   pt_prep_kernel            zero the fixed-point buffer and its flag, gather the contact vertices to world space (R v + t), clamp
//                             scan_point_num to 0 .. S
//   pt_contact_kernel         block per frame: s = sqrt(d + 1e-4), value s / (s + 1), gradient w / (B Nc) / (s + 1)^2 / (2 s) 2 (x - x_nn)
//                             through R^T onto the dverts row the id owns (ids are unique: plain adds)
//   pt_mask_kernel            block per frame: qmask = vis & body_mask and the two counts of the frame rule
//   pt_scan_frame_kernel      block per frame: per-frame GMoF means (rho^2 d / (d + rho^2) on the SQUARED distance, scan.py:188-193); a
//                             valid scan point that is not finite raises the flag (the masked search reports it as "no target")
//   pt_scan_adjoint_kernel    m2s: a gather (a query vertex has one nearest scan point: plain add to its own row); s2m: a scatter
//                             (many scan points share a vertex) into the fixed-point buffer
//   pt_vel_kernel             block per frame, thread per (marker, axis): the [-1, 1] and [1, -2, 1] stencils and their adjoints
//   pt_close_kernel           dverts += the fixed-point sums; block 0 sums the frames and puts the six values into losses[2, 3, 4, 6, 7, 8] and adds them
//                             to losses[0] (a raised flag makes that NaN: the engine's non-finite latch reads it)
// Reproducibility: no fp32 atomic anywhere.  Every loss value is a fixed-order sum (LDS tree per frame in double, then the frames in
// index order); every gradient is either owned by one thread or goes through the fixed-point buffer (fixed_acc.hpp: two 64-bit words
// per entry, units of 2^-20 and 2^-60, contributions below 2^17, sums up to 2^43), whose integer atomics do not depend on the order of arrival.  Graph replay
// equals eager launches bit for bit, and two engines on one window agree bit for bit.
// Every index read from a search result is checked before use: idx = -1 of an invalid query, pairs behind count, ids >= V.
#include "engine_host.hpp"
#include "fixed_acc.hpp"
#include "kernels.hpp"

#include <algorithm>
#include <vector>

namespace lemo {

int selfpen_loss_backward_fixed(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                                int penalize_outside, float gl, long long* acc, int* flag, hipStream_t s);

namespace {

enum { FA_CONTACT = 0, FA_S2M, FA_M2S, FA_ACC, FA_VEL, FA_STRIDE = 8 };
struct PtCam { float R[9], t[3]; };

// fixed-order sum over the 256 threads of a block, the same value in every thread
__device__ __forceinline__ double pt_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ int pt_block_count(int v, int* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256)
pt_prep_kernel(long long* __restrict__ fix, long long nfix, int* __restrict__ flag, const float* __restrict__ verts, int B, int V,
               const int* __restrict__ cvid, int Nc, PtCam cw, float* __restrict__ cxyz, const int* __restrict__ spn, int S,
               int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (fix && i < nfix) fix[i] = 0;
  if (flag && i == 0) *flag = 0;
  if (cvid && i < (long long)B * Nc) {
    const int b = (int)(i / Nc), q = (int)(i - (long long)b * Nc);
    const int vid = cvid[q];
    float w[3] = {0.f, 0.f, 0.f};
    if ((unsigned)vid < (unsigned)V) {
      const float* p = verts + ((size_t)b * V + vid) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = cw.R[3 * k] * p[0] + cw.R[3 * k + 1] * p[1] + cw.R[3 * k + 2] * p[2] + cw.t[k];
    }
    cxyz[3 * i] = w[0]; cxyz[3 * i + 1] = w[1]; cxyz[3 * i + 2] = w[2];
  }
  if (spn && i < B) counts[i] = max(0, min(spn[i], S));
}

__global__ void __launch_bounds__(256)
pt_contact_kernel(const float* __restrict__ cxyz, const float* __restrict__ dist, const int* __restrict__ idx, const float* __restrict__ scene,
                  int M, const int* __restrict__ cvid, int Nc, int V, PtCam cw, float wn, float* __restrict__ dverts,
                  double* __restrict__ frame_acc) {
  __shared__ double red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  double acc = 0.0;
  for (int q = t; q < Nc; q += 256) {
    const size_t i = (size_t)b * Nc + q;
    const float s = sqrtf(dist[i] + 1e-4f);
    acc += (double)(s / (s + 1.0f));
    const int j = idx[i], vid = cvid[q];
    if ((unsigned)j >= (unsigned)M || (unsigned)vid >= (unsigned)V) continue;
    const float coef = wn / ((s + 1.0f) * (s + 1.0f)) / (2.0f * s) * 2.0f;
    float gw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gw[k] = coef * (cxyz[3 * i + k] - scene[3 * (size_t)j + k]);
    float* o = dverts + ((size_t)b * V + vid) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] += cw.R[k] * gw[0] + cw.R[3 + k] * gw[1] + cw.R[6 + k] * gw[2];      // R^T gw
  }
  const double tot = pt_block_sum(acc, red);
  if (t == 0) frame_acc[(size_t)b * FA_STRIDE + FA_CONTACT] = tot;
}

// counts: [0][B] clamped scan_point_num (pt_prep_kernel), [1][B] visible vertices, [2][B] vertices with vis & body_mask
__global__ void __launch_bounds__(256)
pt_mask_kernel(const unsigned char* __restrict__ vis, const unsigned char* __restrict__ body_mask, int B, int V,
               unsigned char* __restrict__ qmask, int* __restrict__ counts) {
  __shared__ int red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  int nv = 0, nq = 0;
  for (int v = t; v < V; v += 256) {
    const bool s = vis[(size_t)b * V + v] != 0, q = s && body_mask[v] != 0;
    qmask[(size_t)b * V + v] = q ? 1 : 0;
    nv += s ? 1 : 0; nq += q ? 1 : 0;
  }
  const int tv = pt_block_count(nv, red);
  const int tq = pt_block_count(nq, red);
  if (t == 0) { counts[B + b] = tv; counts[2 * B + b] = tq; }
}

__device__ __forceinline__ float pt_gmof(float d, float r2) { return r2 * d / (d + r2); }

__global__ void __launch_bounds__(256)
pt_scan_frame_kernel(const float* __restrict__ scan, int S, int B, int V, const int* __restrict__ counts, const unsigned char* __restrict__ qmask,
                     const float* __restrict__ s2m_dist, const float* __restrict__ m2s_dist, float r2s, float r2m, int do_s2m, int do_m2s,
                     int* __restrict__ flag, double* __restrict__ frame_acc) {
  __shared__ double red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = counts[b];
  double a = 0.0, m = 0.0;
  bool bad = false;
  for (int i = t; i < n; i += 256) {
    const float* x = scan + ((size_t)b * S + i) * 3;
    bad = bad || !(fabsf(x[0]) < INFINITY) || !(fabsf(x[1]) < INFINITY) || !(fabsf(x[2]) < INFINITY);
    if (do_s2m) a += (double)pt_gmof(s2m_dist[(size_t)b * S + i], r2s);
  }
  if (bad) *flag = 1;
  if (do_m2s)
    for (int v = t; v < V; v += 256)
      if (qmask[(size_t)b * V + v]) m += (double)pt_gmof(m2s_dist[(size_t)b * V + v], r2m);
  const double ta = pt_block_sum(a, red);
  const double tm = pt_block_sum(m, red);
  if (t == 0) {
    frame_acc[(size_t)b * FA_STRIDE + FA_S2M] = ta / (double)max(n, 1);
    frame_acc[(size_t)b * FA_STRIDE + FA_M2S] = tm / (double)max(counts[2 * B + b], 1);
  }
}

// the frame rule of scan.py:245, 256: a scan point and a visible vertex; m2s also a vertex with vis & body_mask
__device__ __forceinline__ bool pt_live(const int* __restrict__ counts, int B, int b) { return counts[b] > 0 && counts[B + b] > 0; }
__device__ __forceinline__ bool pt_live_m(const int* __restrict__ counts, int B, int b) { return pt_live(counts, B, b) && counts[2 * B + b] > 0; }

// grid (blocks over max(S, V), frame)
__global__ void __launch_bounds__(256)
pt_scan_adjoint_kernel(const float* __restrict__ verts, const float* __restrict__ scan, int B, int V, int S, const int* __restrict__ counts,
                       const unsigned char* __restrict__ qmask, const float* __restrict__ s2m_dist, const int* __restrict__ s2m_idx,
                       const float* __restrict__ m2s_dist, const int* __restrict__ m2s_idx, float ws, float wm, float r2s, float r2m,
                       long long* __restrict__ fix, int* __restrict__ flag, float* __restrict__ dverts) {
  __shared__ float coef[2];
  __shared__ int red[256];
  const int b = blockIdx.y, t = threadIdx.x;
  int ls = 0, lm = 0;
  for (int q = t; q < B; q += 256) { ls += pt_live(counts, B, q) ? 1 : 0; lm += pt_live_m(counts, B, q) ? 1 : 0; }
  ls = pt_block_count(ls, red);
  lm = pt_block_count(lm, red);
  if (t == 0) {
    coef[0] = (ws > 0.f && pt_live(counts, B, b)) ? ws / (float)max(ls, 1) / (float)max(counts[b], 1) : 0.f;
    coef[1] = (wm > 0.f && pt_live_m(counts, B, b)) ? wm / (float)max(lm, 1) / (float)max(counts[2 * B + b], 1) : 0.f;
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + t;
  const float cs = coef[0], cm = coef[1];
  if (cs != 0.f && i < counts[b]) {                        // scan point i pulls its nearest visible vertex
    const int j = s2m_idx[(size_t)b * S + i];
    if ((unsigned)j < (unsigned)V) {
      const float d = s2m_dist[(size_t)b * S + i], den = d + r2s;
      const float g = cs * (r2s * r2s) / (den * den) * 2.0f;
      const float* x = scan + ((size_t)b * S + i) * 3;
      const float* v = verts + ((size_t)b * V + j) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) fix_add(fix, ((size_t)b * V + j) * 3 + k, g * (v[k] - x[k]), flag);
    }
  }
  if (cm != 0.f && i < V && qmask[(size_t)b * V + i]) {    // vertex i is pulled to its nearest valid scan point
    const int j = m2s_idx[(size_t)b * V + i];
    if ((unsigned)j < (unsigned)S) {
      const float d = m2s_dist[(size_t)b * V + i], den = d + r2m;
      const float g = cm * (r2m * r2m) / (den * den) * 2.0f;
      const float* x = scan + ((size_t)b * S + j) * 3;
      const float* v = verts + ((size_t)b * V + i) * 3;
      float* o = dverts + ((size_t)b * V + i) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k] += g * (v[k] - x[k]);
    }
  }
}

// mvel = mk[1:] - mk[:-1]; vel: mean(mvel^2); acc: mean((mvel[1:] - mvel[:-1])^2).  cv = 2 w_vel / ((B-1) n81 3), ca likewise with B-2
__global__ void __launch_bounds__(256)
pt_vel_kernel(const float* __restrict__ verts, int B, int V, const int* __restrict__ row81, int n81, float ca, float cv,
              float* __restrict__ dverts, double* __restrict__ frame_acc) {
  __shared__ double red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  double sa = 0.0, sv = 0.0;
  for (int w = t; w < n81 * 3; w += 256) {
    const int m = w / 3, c = w - 3 * m, vid = row81[m];
    if ((unsigned)vid >= (unsigned)V) continue;
    float x[5];                                            // frames b - 2 .. b + 2, clamped reads
#pragma unroll
    for (int q = 0; q < 5; ++q) x[q] = verts[((size_t)min(max(b + q - 2, 0), B - 1) * V + vid) * 3 + c];
    const float vm2 = x[1] - x[0], vm1 = x[2] - x[1], v0 = x[3] - x[2], v1 = x[4] - x[3];      // mvel[b-2], [b-1], [b], [b+1]
    const float am2 = vm1 - vm2, am1 = v0 - vm1, a0 = v1 - v0;                                  // second differences a[b-2], a[b-1], a[b]
    float g = 0.f;
    if (b < B - 1) { sv += (double)(v0 * v0); g -= cv * v0; }
    if (b >= 1) g += cv * vm1;
    if (b < B - 2) { sa += (double)(a0 * a0); g += ca * a0; }
    if (b >= 1 && b <= B - 2) g -= 2.0f * ca * am1;
    if (b >= 2) g += ca * am2;
    // a vertex listed more than once: its first entry adds every entry's share, in index order
    bool first = true;
    int mult = 0;
    for (int q = 0; q < n81; ++q)
      if (row81[q] == vid) { first = first && q >= m; ++mult; }
    if (!first) continue;
    float* o = dverts + ((size_t)b * V + vid) * 3 + c;
    float cur = *o;
    for (int q = 0; q < mult; ++q) cur += g;
    *o = cur;
  }
  const double ta = pt_block_sum(sa, red);
  const double tv = pt_block_sum(sv, red);
  if (t == 0) { frame_acc[(size_t)b * FA_STRIDE + FA_ACC] = ta; frame_acc[(size_t)b * FA_STRIDE + FA_VEL] = tv; }
}

struct PtClose {
  int B, V, Nc, n81;
  int contact, s2m, m2s, pen, acc, vel;
  float w_contact, w_s2m, w_m2s, w_pen, w_acc, w_vel;
  const int* counts; const float* pen_loss; const double* frame_acc;
  const long long* fix; const int* flag;
  float *dverts, *losses;
};
__global__ void __launch_bounds__(256)
pt_close_kernel(PtClose a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (a.fix && i < (long long)a.B * a.V * 3) {
    const float q = fix_value(a.fix, (size_t)i);
    if (q != 0.f) a.dverts[i] += q;
  }
  if (blockIdx.x != 0) return;
  // block 0: the frames' sums (thread t takes frames t, t + 256, ...; then a fixed tree), the six values by thread 0
  __shared__ double red[256];
  __shared__ int redi[256];
  const int B = a.B, t = threadIdx.x;
  const double* fa = a.frame_acc;
  double sc = 0.0, ss = 0.0, sm = 0.0, sp = 0.0, sa = 0.0, sv = 0.0;
  int ns = 0, nm = 0;
  for (int b = t; b < B; b += 256) {
    if (a.contact) sc += fa[(size_t)b * FA_STRIDE + FA_CONTACT];
    if (a.s2m && pt_live(a.counts, B, b)) { ss += fa[(size_t)b * FA_STRIDE + FA_S2M]; ++ns; }
    if (a.m2s && pt_live_m(a.counts, B, b)) { sm += fa[(size_t)b * FA_STRIDE + FA_M2S]; ++nm; }
    if (a.pen) sp += (double)(a.w_pen * a.pen_loss[b]);
    if (a.acc) sa += fa[(size_t)b * FA_STRIDE + FA_ACC];
    if (a.vel) sv += fa[(size_t)b * FA_STRIDE + FA_VEL];
  }
  sc = pt_block_sum(sc, red); ss = pt_block_sum(ss, red); sm = pt_block_sum(sm, red);
  sp = pt_block_sum(sp, red); sa = pt_block_sum(sa, red); sv = pt_block_sum(sv, red);
  ns = pt_block_count(ns, redi); nm = pt_block_count(nm, redi);
  if (t != 0) return;
  const float contact = a.contact ? a.w_contact * (float)(sc / ((double)B * a.Nc)) : 0.f;
  const float s2m = a.s2m ? a.w_s2m * (float)(ss / (double)max(ns, 1)) : 0.f;
  const float m2s = a.m2s ? a.w_m2s * (float)(sm / (double)max(nm, 1)) : 0.f;
  const float pen = a.pen ? (float)sp : 0.f;
  const float acc = a.acc ? a.w_acc * (float)(sa / ((double)(B - 2) * a.n81 * 3)) : 0.f;
  const float vel = a.vel ? a.w_vel * (float)(sv / ((double)(B - 1) * a.n81 * 3)) : 0.f;
  // ProxTemporalFitter.loss_dict's order of additions behind the S2 / S3 terms
  float total = a.losses[0];
  total += contact; total += (s2m + m2s); total += pen; total += acc; total += vel;
  if (a.flag && *a.flag) total = NAN;                      // a contribution that could not be converted: the latch has to see it
  a.losses[0] = total; a.losses[2] = s2m; a.losses[3] = m2s; a.losses[4] = pen; a.losses[6] = contact; a.losses[7] = acc; a.losses[8] = vel;
}

bool weight_ok(float w) { return std::isfinite(w) && w >= 0.f; }

}  // namespace

// which terms an attached descriptor switches on
struct PtLive { bool contact, s2m, m2s, pen, acc, vel; bool scan() const { return s2m || m2s; } bool fix() const { return s2m || pen; }
                bool any() const { return contact || s2m || m2s || pen || acc || vel; } };
static PtLive pt_live_terms(const lemo_prox_terms& t) {
  PtLive l;
  l.contact = t.contact_loss_weight > 0.f && t.scene_v && t.contact_vid;
  const bool scan = t.scan && t.scan_point_num && t.body_mask && t.faces;
  l.s2m = scan && t.s2m_weight > 0.f;
  l.m2s = scan && t.m2s_weight > 0.f;
  l.pen = t.coll_loss_weight > 0.f && t.faces;
  l.acc = t.smooth_acc_weight > 0.f;
  l.vel = t.smooth_vel_weight > 0.f;
  return l;
}

int prox_terms_check(const lemo_prox_desc& d, const lemo_prox_terms& t) {
  for (float w : {t.contact_loss_weight, t.s2m_weight, t.m2s_weight, t.coll_loss_weight, t.smooth_acc_weight, t.smooth_vel_weight})
    if (!weight_ok(w)) return LEMO_ERR_ARG;
  const PtLive l = pt_live_terms(t);
  const int B = d.B, V = d.V;
  if (l.any() && !t.frame_acc) return LEMO_ERR_ARG;
  if (l.fix() && (!t.fix_acc || !t.fix_flag)) return LEMO_ERR_ARG;
  if (l.scan() && !t.fix_flag) return LEMO_ERR_ARG;
  if (l.contact) {
    if (t.Nc < 1 || t.M < 1) return LEMO_ERR_SHAPE;
    const long long need = lemo_chamfer_workspace_bytes(B, t.Nc, t.M, LEMO_CHAMFER_SHARED, 0);
    if (need < 0) return LEMO_ERR_SHAPE;
    if (!t.contact_vid_host || !t.contact_xyz || !t.contact_dist || !t.contact_idx || t.contact_ws_bytes < need || (need > 0 && !t.contact_ws))
      return LEMO_ERR_ARG;
    std::vector<int> ids(t.contact_vid_host, t.contact_vid_host + t.Nc);
    std::sort(ids.begin(), ids.end());
    if (ids.front() < 0 || ids.back() >= V || std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return LEMO_ERR_ARG;
  }
  if (l.scan()) {
    if (t.S < 1 || t.F < 1) return LEMO_ERR_SHAPE;
    const long long nv = lemo_vertex_visibility_workspace_bytes(B, V, t.F, LEMO_VIS_AUTO, 0);
    const long long n1 = lemo_chamfer_workspace_bytes(B, t.S, V, 0, 0), n2 = lemo_chamfer_workspace_bytes(B, V, t.S, 0, 0);
    if (nv < 0 || n1 < 0 || n2 < 0) return LEMO_ERR_SHAPE;
    const long long ns = std::max(n1, n2);
    if (!(t.rho_s2m > 0.f) || !(t.rho_m2s > 0.f) || !std::isfinite(t.rho_s2m) || !std::isfinite(t.rho_m2s) || !(t.min_dist >= 0.f) ||
        !std::isfinite(t.min_dist))
      return LEMO_ERR_ARG;
    if (!t.vis || !t.qmask || !t.scan_counts || !t.s2m_dist || !t.s2m_idx || !t.m2s_dist || !t.m2s_idx || t.vis_ws_bytes < nv ||
        (nv > 0 && !t.vis_ws) || t.scan_ws_bytes < ns || (ns > 0 && !t.scan_ws))
      return LEMO_ERR_ARG;
  }
  if (l.pen) {
    if (t.F < 1 || t.max_pairs < 1) return LEMO_ERR_SHAPE;
    const long long np = lemo_selfpen_search_workspace_bytes(B, V, t.F, LEMO_SELFPEN_AUTO, 0);
    if (np < 0 || (long long)B * t.max_pairs > (1ll << 28)) return LEMO_ERR_SHAPE;
    if (!(t.sigma > 0.f) || !std::isfinite(t.sigma) || t.P < 0 || t.P > 64 || (t.ign && t.P < 1) || (!t.ign && t.P != 0) ||
        ((t.parents || t.ign) && !t.segm))
      return LEMO_ERR_ARG;
    if (!t.pairs || !t.pair_count || !t.pen_loss || !t.pen_ws || t.pen_ws_bytes < np) return LEMO_ERR_ARG;
  }
  if ((l.acc || l.vel) && (!d.fit.row81 || d.fit.n81 < 1)) return LEMO_ERR_ARG;
  return 0;
}

bool prox_terms_any(const lemo_prox_terms& t) { return pt_live_terms(t).any(); }

// the launches of one iteration: behind prox_sparse (losses[] finalised, dverts holds the S2 / S3 gradient), in front of lbs_verts_bwd
int prox_terms_run(const lemo_prox_desc& d, const lemo_prox_terms& t, hipStream_t s) {
  const PtLive l = pt_live_terms(t);
  if (!l.any()) return 0;
  const int B = d.B, V = d.V;
  const long long nsum = l.fix() ? (long long)B * V * 3 : 0, nfix = LEMO_FIX_WORDS * nsum;      // destinations, words to zero
  PtCam cw;
  for (int i = 0; i < 9; ++i) cw.R[i] = d.cam2world[i];
  for (int i = 0; i < 3; ++i) cw.t[i] = d.cam2world[9 + i];
  const dim3 blk(256);
  {
    const long long n = std::max<long long>({nfix, l.contact ? (long long)B * t.Nc : 0, (long long)B, 1});
    hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((n + 255) / 256)), blk, 0, s, l.fix() ? t.fix_acc : nullptr, nfix, t.fix_flag, d.verts, B, V,
                       l.contact ? t.contact_vid : nullptr, t.Nc, cw, t.contact_xyz, l.scan() ? t.scan_point_num : nullptr, t.S, t.scan_counts);
  }
  if (l.contact) {
    CHK(lemo_chamfer_forward(t.contact_xyz, t.scene_v, B, t.Nc, t.M, LEMO_CHAMFER_SHARED, 0, t.contact_dist, t.contact_idx, nullptr, nullptr,
                             t.contact_ws, t.contact_ws_bytes, s));
    const float wn = (float)((double)t.contact_loss_weight / ((double)B * t.Nc));
    hipLaunchKernelGGL(pt_contact_kernel, dim3(B), blk, 0, s, t.contact_xyz, t.contact_dist, t.contact_idx, t.scene_v, t.M, t.contact_vid, t.Nc, V,
                       cw, wn, d.dverts, t.frame_acc);
  }
  if (l.scan()) {
    const float r2s = t.rho_s2m * t.rho_s2m, r2m = t.rho_m2s * t.rho_m2s;
    CHK(lemo_vertex_visibility(d.verts, B, V, t.faces, t.F, nullptr, t.min_dist, LEMO_VIS_AUTO, 0, t.vis, nullptr, t.vis_ws, t.vis_ws_bytes, s));
    hipLaunchKernelGGL(pt_mask_kernel, dim3(B), blk, 0, s, t.vis, t.body_mask, B, V, t.qmask, t.scan_counts);
    if (l.s2m)
      CHK(lemo_chamfer_masked_forward(t.scan, d.verts, B, t.S, V, t.scan_counts, nullptr, nullptr, t.vis, 0, t.s2m_dist, t.s2m_idx, t.scan_ws,
                                      t.scan_ws_bytes, s));
    if (l.m2s)
      CHK(lemo_chamfer_masked_forward(d.verts, t.scan, B, V, t.S, nullptr, t.qmask, t.scan_counts, nullptr, 0, t.m2s_dist, t.m2s_idx, t.scan_ws,
                                      t.scan_ws_bytes, s));
    hipLaunchKernelGGL(pt_scan_frame_kernel, dim3(B), blk, 0, s, t.scan, t.S, B, V, t.scan_counts, t.qmask, t.s2m_dist, t.m2s_dist, r2s, r2m,
                       l.s2m ? 1 : 0, l.m2s ? 1 : 0, t.fix_flag, t.frame_acc);
    hipLaunchKernelGGL(pt_scan_adjoint_kernel, dim3((std::max(t.S, V) + 255) / 256, B), blk, 0, s, d.verts, t.scan, B, V, t.S, t.scan_counts, t.qmask,
                       t.s2m_dist, t.s2m_idx, t.m2s_dist, t.m2s_idx, l.s2m ? t.s2m_weight : 0.f, l.m2s ? t.m2s_weight : 0.f, r2s, r2m, t.fix_acc,
                       t.fix_flag, d.dverts);
  }
  if (l.pen) {
    CHK(lemo_selfpen_search(d.verts, B, V, t.faces, t.F, t.segm, t.parents, t.ign, t.P, LEMO_SELFPEN_AUTO, 0, t.pairs, t.max_pairs, t.pair_count,
                            t.pen_ws, t.pen_ws_bytes, s));
    CHK(lemo_selfpen_loss_forward(d.verts, B, V, t.faces, t.F, t.pairs, t.max_pairs, t.pair_count, t.sigma, t.penalize_outside, t.pen_loss, s));
    CHK(selfpen_loss_backward_fixed(d.verts, B, V, t.faces, t.F, t.pairs, t.max_pairs, t.pair_count, t.sigma, t.penalize_outside,
                                    t.coll_loss_weight, t.fix_acc, t.fix_flag, s));
  }
  const int n81 = d.fit.n81;
  if (l.acc || l.vel) {
    const float ca = l.acc ? (float)(2.0 * (double)t.smooth_acc_weight / ((double)(B - 2) * n81 * 3)) : 0.f;
    const float cv = l.vel ? (float)(2.0 * (double)t.smooth_vel_weight / ((double)(B - 1) * n81 * 3)) : 0.f;
    hipLaunchKernelGGL(pt_vel_kernel, dim3(B), blk, 0, s, d.verts, B, V, d.fit.row81, n81, ca, cv, d.dverts, t.frame_acc);
  }
  PtClose c{};
  c.B = B; c.V = V; c.Nc = t.Nc; c.n81 = n81;
  c.contact = l.contact; c.s2m = l.s2m; c.m2s = l.m2s; c.pen = l.pen; c.acc = l.acc; c.vel = l.vel;
  c.w_contact = t.contact_loss_weight; c.w_s2m = t.s2m_weight; c.w_m2s = t.m2s_weight; c.w_pen = t.coll_loss_weight;
  c.w_acc = t.smooth_acc_weight; c.w_vel = t.smooth_vel_weight;
  c.counts = t.scan_counts; c.pen_loss = t.pen_loss; c.frame_acc = t.frame_acc;
  c.fix = l.fix() ? t.fix_acc : nullptr; c.flag = t.fix_flag; c.dverts = d.dverts; c.losses = d.losses;
  hipLaunchKernelGGL(pt_close_kernel, dim3((unsigned)((std::max<long long>(nsum, 1) + 255) / 256)), blk, 0, s, c);
  return (int)hipGetLastError();
}

}  // namespace lemo
