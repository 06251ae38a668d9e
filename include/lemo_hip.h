/* lemo_hip.h -- C ABI of liblemo_hip.so, the MI355X (gfx950) kernels of LEMO's temporal fitting hot path.
 *
 * The reference (sanweiliti/LEMO) has no native/FFI layer: its boundary for this path is the Python
 * object API of smplx / VPoser / Enc.  This header is the boundary the build adds
 * underneath those objects; each entry point names the reference code whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers to DEVICE memory + sizes; the caller owns every buffer (the Python host side
 *     allocates them with torch); nothing here allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it;
 *   - return 0 on success, a hipError_t value or LEMO_ERR_* (>= 10001) otherwise;
 *   - fp32 everywhere (the reference path is fp32; the 1e6-weighted smoothness loss forbids less).
 */
#ifndef LEMO_HIP_H
#define LEMO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif
/* liblemo_hip.so is built with -fvisibility=hidden: the declarations of this header are its ONLY exports (tests/test_abi.py
 * compares `nm -D` with the prototypes below). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define LEMO_ERR_SHAPE 10001
#define LEMO_ERR_ARG 10002
#define LEMO_ERR_STATE 10003

int lemo_abi_version(void);
/* bit 0: built with -fno-slp-vectorize -fno-vectorize (csrc/Makefile passes -DLEMO_NO_PACKED_FP32 together with them): no
 * auto-vectorised packed fp32, the co-residency hazard of DESIGN 9.3.  lemo_amd._hip refuses a library without it. */
int lemo_build_flags(void);

/* ---- motion-smoothness encoder, models/AE_sep.py:11-30,77-99 (Enc(downsample=False)) ----------
 * Activations: CG8P layout act[C/8][(H+2)*(W+2)][8], zero 1-pixel border owned by the caller.
 * Weights: wt[tap][Cin/8][Cout][8] (packed by lemo_amd.priors.pack_conv3x3 / pack_conv3x3_bwd). */
/* epi 0: out = lrelu(conv + bias) | 1: out = conv * lrelu'(aux) (backward-data) | 2: out = conv + bias
 * variant 0: 4 waves x (32 px x Cout) per block | 1: CU-balanced geometry (256 full blocks + fine tail) */
int lemo_conv3x3_mfma(const float* in, const float* wt, const float* bias, const float* aux, float* out,
                      int H, int W, int cin, int cout, int epi, int variant, void* stream);
/* LDS-tiled variant (the engine's default): additionally takes the channel-group-major pack
 * wt2[Cin/8][tap][Cout][8]; W must satisfy 127 + 2*(127/W+1) + 2*(W+2) + 3 <= 416 (W <= 139) */
/* variant 0 with the K = 9 Cin reduction split over `ks` slices (grid.z) + a combine pass; for layers with few pixels
 * and many channels (too few tiles to fill the chip).  partial: ks * (cout/8) * (H+2)*(W+2) * 8 floats of scratch. */
int lemo_conv3x3_mfma_splitk(const float* in, const float* wt, const float* bias, const float* aux, float* out,
                             float* partial, int ks, int H, int W, int cin, int cout, int epi, void* stream);
int lemo_conv3x3_mfma_lds(const float* in, const float* wt, const float* wt2, const float* bias, const float* aux,
                          float* out, int H, int W, int cin, int cout, int epi, void* stream);
/* diagnostics: same launch (epi 0, Cout % 64 == 0) that also records, per wave, {HW_ID, XCC_ID, start, end}
 * shader-clock stamps into dbg[(block*8 + wave)*4 ..] -- used by tools/conv_census.py only */
int lemo_conv3x3_mfma_lds_census(const float* in, const float* wt, const float* wt2, const float* bias, float* out,
                                 int H, int W, int cin, int cout, unsigned long long* dbg, void* stream);
/* variant 3 ("split-bf16"): the same fp32 convolution for Cin, Cout in {32, 64} on the bf16 matrix cores.  Each fp32
 * operand is split exactly into three bf16 pieces and six of the nine piece products are accumulated in fp32
 * (error of the dropped terms < 2^-24 per product, 100x below the fp32 accumulation rounding of any fp32 conv).
 * w3 = weights pre-split on the host: bf16 w3[Cin/16][tap 9][Cout/32][split 3][lane 64][8] with lane l holding
 * cout (l&31) of the 32-block and channels 8*(2*kc + (l>>5)) .. +7; wt = the tap-major fp32 pack (remainder pixels).
 * Returns LEMO_ERR_SHAPE for shapes it does not take (lemo_conv3x3_split_supported() == 0). */
int lemo_conv3x3_split_supported(int H, int W, int cin, int cout);
int lemo_conv3x3_mfma_split(const float* in, const void* w3, const float* wt, const float* bias, const float* aux,
                            float* out, int H, int W, int cin, int cout, int epi, void* stream);
int lemo_conv3x3_mfma_split_census(const float* in, const void* w3, const float* wt, const float* bias, float* out,
                                   int H, int W, int cin, int cout, unsigned long long* dbg, void* stream);
/* variant 4 ("split-f16", the engines' default since round 3): the same convolution with TWO fp16 pieces per operand and
 * three of the four piece products (the error-compensated fp16 scheme of Markidis et al. / Ootomo & Yokota: hi = f16(x s),
 * lo = f16(x s - hi); a b ~= a_hi b_lo + a_lo b_hi + a_hi b_hi, fp32 accumulate) -- half the matrix-core work of variant 3,
 * error vs float64 at the level of an fp32 convolution (conv_split_kernels.hip header has the measurements).  The
 * activations are scaled per workgroup inside the kernel (any fp32 CG8P tensor is a valid input); the weights are scaled
 * on the host: w2 = f16 w2[Cin/16][tap 9][Cout/32][piece 2][lane 64][8] of weight * 2^k, winv = 2^-k. */
int lemo_conv3x3_mfma_split_f16(const float* in, const void* w2, float winv, const float* wt, const float* bias, const float* aux,
                                float* out, int H, int W, int cin, int cout, int epi, void* stream);
/* census of either variant (pieces = 3: w = w3, winv ignored; pieces = 2: w = w2) */
int lemo_conv3x3_mfma_split_census2(const float* in, const void* w, float winv, int pieces, const float* wt, const float* bias, float* out,
                                    int H, int W, int cin, int cout, unsigned long long* dbg, void* stream);
/* variant 5 ("pairs", the engines' default since round 4): TWO consecutive 64 -> 64 layers of the encoder in ONE launch, in the
 * arithmetic of variant 4.  A workgroup owns a 10 x 14 output tile, stages the 14 x 18 input tile once, keeps the 12 x 16
 * intermediate tile in LDS (zero outside the image = the second layer's padding) and never re-reads it from HBM:
 *   epi 0 (forward, models/AE_sep.py:11-30): mid = lrelu(conv(in, A) + biasA), out = lrelu(conv(mid, B) + biasB); `mid` (all 64
 *          channels, CG8P) is ALSO written -- the backward pass needs every layer's activation;
 *   epi 1 (backward-data): mid = conv(in, A) * lrelu'(auxA), out = conv(mid, B) * lrelu'(auxB) with A / B the backward packs of the
 *          LATER / EARLIER layer and auxA / auxB the saved activations at the mid / out positions; `mid` is not written.
 * wA / wB: the variant-4 packs (pack_conv3x3_split_f16 / pack_conv3x3_bwd_split_f16), winvA / winvB their inverse host scales.
 * dbg (epi 0 only, may be NULL): per wave {HW_ID, XCC_ID, start, end, after staging, after layer 1, after the mid planes} stamps. */
int lemo_conv3x3_pair_supported(int H, int W, int c0, int c1, int c2);
int lemo_conv3x3_pair_f16(const float* in, const void* wA, float winvA, const float* biasA, const float* auxA, float* mid,
                          const void* wB, float winvB, const float* biasB, const float* auxB, float* out, int H, int W, int epi,
                          unsigned long long* dbg, void* stream);
/* The encoder's turn (conv variant 9's step schedule, csrc/conv_turn_kernels.hip): layer 9 forward, the latent smoothness loss
 * gradient and layer 9 backward-data in ONE launch, on 12 x 12 output tiles with everything between the two convolutions in LDS:
 *   z = lrelu(conv(in, wf) + bias) (the owned pixels written to z, CG8P 64 channels: act[10]);
 *   d(pre-act 10) = coef2 * 2-sided time difference of z * lrelu'(z), zero outside the image (lemo_smooth_loss's arithmetic: for
 *     equal z the values are bit-identical);
 *   out = conv^T(d(pre-act 10), wb) * lrelu'(in) (d(pre-act 9)).
 * wf / wb: pack_conv3x3_split_f16 / pack_conv3x3_bwd_split_f16 of layer 9, winvf / winvb their inverse host scales.  acc (may be
 * NULL): f64 [32][16]; every workgroup adds its sum of (z[x+1] - z[x])^2 over its owned pixels and channels to acc[(wg & 31) * 16].
 * dpre (may be NULL): receives d(pre-act 10) of every image pixel (CG8P).  dbg (may be NULL): per wave {HW_ID, start, after staging,
 * after layer 9 forward, after the stencil, after the dpre planes, end} stamps; ceil(H / 12) * ceil(W / 12) workgroups x 8 waves x 8.
 * Refuses W < 2 (no time difference). */
int lemo_conv3x3_turn_supported(int H, int W);
int lemo_conv3x3_turn_f16(const float* in, const void* wf, float winvf, const float* bias, const void* wb, float winvb, float* z, float* out,
                          double* acc, float coef2, int H, int W, float* dpre, unsigned long long* dbg, void* stream);
/* variant 10 (round 6): ONE 64 -> 64 layer (forward, epi 0, models/AE_sep.py:11-30; backward-data, epi 1) as a Winograd F(2x2, 3x3)
 * convolution: 16 instead of 36 multiplies per 2 x 2 output tile and (cin, cout), the 16 [64 x 64 x tiles] GEMMs in the split-f16
 * arithmetic of variant 4 (fp32 transforms, two fp16 pieces per operand, 3 MFMA products, fp32 accumulate).  A workgroup owns 32
 * consecutive 2 x 2 tiles of the even part of the image; the last row of an odd H is a direct fp32 convolution from `wt`.
 * wU = pack_conv3x3_wino_f16 / pack_conv3x3_bwd_wino_f16 (G g G^T in float64, split on the host; winv = its inverse scale),
 * wt = the fp32 tap-major pack of the same weights (pack_conv3x3 / pack_conv3x3_bwd).  dbg (epi 0 only, may be NULL): per wave
 * {start, loads issued, transformed, planes written, GEMMs done, exchanged, end, HW_ID} shader-clock stamps (tools/wino_check.py). */
int lemo_conv3x3_wino_supported(int H, int W, int cin, int cout);
int lemo_conv3x3_wino_f16(const float* in, const void* wU, float winv, const float* wt, const float* bias, const float* aux, float* out,
                          int H, int W, int epi, unsigned long long* dbg, void* stream);
/* first layer, 1 input channel: x0 padded [(H+2)*(W+2)], w [Cout][9] */
int lemo_conv3x3_c1(const float* x0, const float* w, const float* bias, float* out, int H, int W, int cout, void* stream);
int lemo_conv3x3_c1_bwd(const float* dpre, const float* w, float* dx0, int H, int W, int cout, void* stream);
/* loss_smooth = mean((z[...,1:]-z[...,:-1])^2)  (opt_amass_temp.py:390-391) fused with d(loss)/d(pre-act):
 * partial[lemo_smooth_loss_blocks()] receives per-block sums of squares; coef2 = weight*2/count.  z, dpre: CG8P; the border
 * of z is loaded but never used, the border of dpre is not written.  LEMO_ERR_SHAPE for H < 1, W < 1, C < 8 or C % 8,
 * LEMO_ERR_ARG for a null z or dpre */
int lemo_smooth_loss_blocks(int H, int W, int C);
int lemo_smooth_loss(const float* z, float* dpre, float* partial, int H, int W, int C, float coef2, void* stream);

/* ---- VPoser.decode, human_body_prior/train/vposer_smpl.py:107-121 ------------------------------ */
typedef struct lemo_vposer_w {           /* *_t = transposed copy [in][out]; the out layer is zero-padded 126 -> 128 */
  const float *w1, *w1t, *b1;            /* bodyprior_dec_fc1  [512][32]  / [32][512]  / [512] */
  const float *w2, *w2t, *b2;            /* bodyprior_dec_fc2  [512][512] / [512][512] / [512] */
  const float *w3, *w3t, *b3;            /* bodyprior_dec_out  [128][512] / [512][128] / [128] */
} lemo_vposer_w;
int lemo_vposer_decode_fwd(const lemo_vposer_w* w, const float* z, int z_stride, int B, float* h1, float* h2, float* o,
                           float* matrot, float* aa, void* stream);
/* scratch: [B][1152] floats */
int lemo_vposer_decode_bwd(const lemo_vposer_w* w, const float* h1, const float* h2, const float* o, const float* d_aa,
                           const float* d_matrot, int B, float* dz, int dz_stride, float* scratch, void* stream);
/* MLP part of the VPoser backward alone: dout [B][128] (= scratch[0 .. B*128)) -> dz */
int lemo_vposer_mlp_bwd(const lemo_vposer_w* w, const float* h1, const float* h2, int B, float* dz, int dz_stride,
                        float* scratch, void* stream);
/* ---- VPoser.encode in eval mode, human_body_prior/train/vposer_smpl.py:98-105, forward and input gradient (csrc/vposer_enc_kernels.hip)
 * x [B][63] -> bn1 -> fc1 -> lrelu -> bn2 -> fc2 -> lrelu -> mean = mu(h2), std = softplus(logvar(h2)).  BatchNorm (running statistics,
 * eps 1e-5) is folded into the next layer on the host, in float64: fc1' = fc1 diag(s1), b1' = b1 + fc1 t1 with s = gain / sqrt(var + eps),
 * t = shift - mean s; fc2' likewise with bn2.  The two heads are one [64][512] layer: mu rows 0..31, logvar rows 32..63. */
typedef struct lemo_vposer_enc_w {       /* *p = fragment-order pack P[K/16][M/16][64][4] of a row-major [M][K] matrix: lane 16 q + i of
                                          * (chunk c, tile mt) holds W[16 mt + i][16 c + 4 q .. + 3]; *tp = the same pack of the transpose */
  const float *w1p, *w1tp, *b1;          /* bn1 + bodyprior_enc_fc1  [512][64] (column 63 zero) / [64][512] (row 63 zero) / [512] */
  const float *w2p, *w2tp, *b2;          /* bn2 + bodyprior_enc_fc2  [512][512] / [512][512] / [512] */
  const float *whp, *whtp, *bh;          /* bodyprior_enc_mu | bodyprior_enc_logvar  [64][512] / [512][64] / [64] */
} lemo_vposer_enc_w;
/* pin: B rows of 63 floats, pin_stride >= 63 floats apart (column 63 is never read); mean, std: B rows of 32, out_stride >= 32 apart; nothing
 * outside those columns is read or written.  h1, h2 [B][512] and lv [B][32] (the pre-softplus logvar output), 16-byte aligned, are what the
 * backward needs; each may be NULL (not saved).  LEMO_ERR_ARG, nothing written: B <= 0, a null w / pin / mean / std, pin_stride < 63,
 * out_stride < 32. */
int lemo_vposer_encode_fwd(const lemo_vposer_enc_w* w, const float* pin, int pin_stride, int B, float* mean, float* std, int out_stride,
                           float* h1, float* h2, float* lv, void* stream);
/* d_mean, d_std: B rows of 32, out_stride apart; either may be NULL (= zero).  dpin: B rows of 63 written, pin_stride apart.  LEMO_ERR_ARG,
 * nothing written: B <= 0, a null w / h1 / h2 / lv / dpin, pin_stride < 63, out_stride < 32.  Parameter gradients are not computed. */
int lemo_vposer_encode_bwd(const lemo_vposer_enc_w* w, const float* h1, const float* h2, const float* lv, const float* d_mean,
                           const float* d_std, int out_stride, int B, float* dpin, int pin_stride, void* stream);
/* generic small NT GEMM on the matrix cores: C[n][m] = epi(sum_k A[m][k] B[n][k]); M, K multiples of 16 */
int lemo_gemm_nt16(const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc,
                   const float* bias, const float* aux, int ldaux, int epi, void* stream);
/* long-K form of the same contraction (M x N <= 512 x 128 outputs, K in the tens of thousands: the feature gradient of the
   all-vertex LBS backward, lbs.py:94-99 transposed): K slabs on the bf16 matrix cores with exactly split fp32 operands, partial
   tiles reduced in slab order (deterministic).  part: lemo_gemm_nt16_splitk_part_floats(M, S) floats of scratch;
   A_grouped: optional copy of A as [K/16][M][16] (contiguous operand tiles); N <= 128, M % 64 == 0, K % 16 == 0 */
int lemo_gemm_nt16_splitk_part_floats(int M, int S);
int lemo_gemm_nt16_splitk(const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc, float* part, int S,
                          const float* A_grouped, void* stream);
/* convert_to_3D_rot's 6-D -> axis-angle, utils/utils.py:111-123 (+63-81) */
int lemo_rot6d_to_aa_fwd(const float* x6, int stride, int N, float* aa, void* stream);
int lemo_rot6d_to_aa_bwd(const float* x6, int stride, const float* d_aa, int N, float* dx6, void* stream);

/* ---- SMPL-X pose stage: smplx==0.1.26 SMPLX.forward + lbs.py:81-106,166-263 --------------------- */
typedef struct lemo_body_const {
  int nj, nshape, ncomp, nlev;
  const int *parents, *level_start, *level_joints, *child_start, *child_list;
  const float *J_template, *J_dirs, *pose_mean, *lh_comp, *rh_comp;
} lemo_body_const;
typedef struct lemo_pose_in {
  const float *global_orient, *body_pose, *jaw, *leye, *reye, *lh, *rh;
  int hand_stride;
  const float* betas;
  int betas_stride;
  const float* expr;
  /* optional fused producers (fitting engine): when non-null they replace global_orient / body_pose */
  const float* rot6d;        /* [B][6]  -> global_orient = 6-D -> axis-angle (utils/utils.py:111-123) */
  const float* vposer_o;     /* [B][128] VPoser out layer -> body_pose = 21 x (6-D -> aa) */
  float* go_out;             /* [B][3] receives the global_orient derived from rot6d */
  /* optional per-iteration bookkeeping done by block 0: zero n_zero doubles, latch the step counter */
  double* zero_f64;
  int n_zero;
  const int* step_ctr;
  int* step_cur;
  int* nonfinite;            /* optional [2]: block 0 latches nonfinite[1] = nonfinite[0] (see lemo_fit_desc.nonfinite) */
} lemo_pose_in;
typedef struct lemo_pose_ws {
  float *full_pose, *R, *J, *T, *A, *Jtr, *Xg;
  int Bp;
  unsigned short* XgS;   /* optional [512/16][3][Bp][2][8] bf16: Xg split into its three exact bf16 pieces, in the fragment order of
                            lemo_lbs_verts_fwd_xs's blend GEMM (written by lemo_smplx_pose_fwd when non-NULL; pad entries stay 0) */
  int xgs_f16;           /* 1: XgS holds TWO fp16 pieces instead, [512/16][2][Bp][2][8] (hi = f16(x), lo = f16(x - hi)): the B operand
                            of the blend GEMM on the fp16 matrix cores; goes with lemo_skin_const.DgH (both or neither) */
} lemo_pose_ws;
typedef struct lemo_pose_grad_in {
  const float *dA, *dJtr, *dX;
  const float* d_full_pose;  /* optional [B][3 nj]: extra d(loss)/d(full_pose) added before the pose chain (PROX angle prior) */
} lemo_pose_grad_in;
typedef struct lemo_pose_grad_out {
  float *d_global_orient, *d_body_pose, *d_jaw, *d_leye, *d_reye, *d_lh, *d_rh;
  int hand_stride;
  float *d_betas, *d_expr;
  /* optional fused consumers (fitting engine) */
  const float* rot6d;        /* [B][6] with d_rot6d: chain d(global_orient) back to the 6-D parameters */
  float* d_rot6d;            /* [B][6] */
  const float* vposer_o;     /* [B][128] with d_vposer_o: chain d(body_pose) back to the VPoser out layer */
  float* d_vposer_o;         /* [B][128] */
} lemo_pose_grad_out;
int lemo_smplx_pose_fwd(const lemo_body_const* c, const lemo_pose_in* in, const lemo_pose_ws* ws, int B, void* stream);
int lemo_smplx_pose_bwd(const lemo_body_const* c, const lemo_pose_ws* ws, const lemo_pose_grad_in* gi,
                        const lemo_pose_grad_out* go, int B, void* stream);

/* ---- SMPL-X vertex stage (blend shapes + skinning + transl): lbs.py:81,94-99,108-117 ------------ */
typedef struct lemo_skin_const {
  int V, NC, KW;
  int blend_fp32;           /* blend GEMM of lemo_lbs_verts_fwd: 0 (default) = bf16 matrix cores with exact fp32 operands
                             * (3-way bf16 split, 6 products, fp32 accumulate -- same error class as an fp32 GEMM, see
                             * lemo_conv3x3_mfma_split) ; 1 = fp32-input MFMA.  Per model constant: no process-wide state */
  const float* Dg;          /* [64][NC][8]  blend directions (shape | pose), K padded to 512 */
  const float* v_template;  /* [V][3] */
  const int* w_idx;         /* [V][KW] ELL skinning weights */
  const float* w_val;
  const unsigned short* DgH; /* optional: Dg * 2^k pre-split on the host into two fp16 pieces, [64][NC][2 halves][hi 4 | lo 4] (the same
                             * 32 bytes per (8-feature group, column) as Dg: HBM sees the same traffic, the kernel converts nothing).
                             * With it (and blend_fp32 == 0, XgS in its fp16 form) the blend GEMM is 3 fp16 MFMA products per 16-deep
                             * k-chunk (hi hi + hi lo + lo hi: operands carried to 2^-22, fp32 accumulate) instead of 6 bf16 ones. */
  float dgh_inv;            /* 2^-k */
} lemo_skin_const;
typedef struct lemo_vertex_set_bwd {
  int n, NCs;
  const int *ids, *vp_row;
  const float* Dk;          /* [512][NCs] */
  const float* DkT;         /* [NCs][512]: the same directions feature-contiguous (forward over the set), or NULL */
  const int *jcsr_start, *jcsr_u;
  const float* jcsr_w;
  /* optional (large sets): deterministic dense backward.  Chunk c (512 consecutive set positions) owns the entries
   * jcsr_chunk[c * (nj + 1) + j] .. jcsr_chunk[c * (nj + 1) + j + 1] of jc_u / jc_w for joint j;
   * part: [part_frames][n_chunk][nj * 12 + 4] floats of per-chunk partial sums, reduced in chunk order. */
  const int* jcsr_chunk;          /* [n_chunk * (nj + 1)] offsets into jc_u / jc_w, or NULL */
  const int* jc_u;                /* the same (set position, weight) pairs as jcsr_u / jcsr_w, reordered CHUNK-major (chunk, */
  const float* jc_w;              /* then joint, then position): the entries of one 512-vertex chunk are one contiguous run */
  float* part;
  int part_frames;
  /* optional: K-slab partial tiles of the feature-gradient GEMM dX = Dk . d(v_posed) (K = NCs): gemm_slabs x 128 x 512
   * floats; when NULL the one-workgroup-per-output-tile GEMM is used (fine for the compact sets, 107 us for all vertices) */
  int gemm_slabs;
  float* gemm_part;
  const float* DkG;         /* optional, with gemm_part: Dk again as [NCs/16][512][16] (k-chunk major: the 64-row x 16-k operand tile of a
                               split-K step is one contiguous 4 KB run instead of 64 segments 4 NCs bytes apart) */
} lemo_vertex_set_bwd;
int lemo_lbs_verts_fwd(const lemo_skin_const* c, const float* Xg, int Bp, const float* A, int nj, const float* transl,
                       const int* ids, int n, int B, float* verts, float* v_posed, void* stream);
/* diagnostics (tools/lbs_census.py): same launch, per wave {start, after prologue, after GEMM, end} clock stamps */
/* same, with the per-frame features also given pre-split (lemo_pose_ws.XgS): the blend GEMM reads its B operand from there.
 * XgS must be in the form c selects: two fp16 pieces when c->DgH is set (lemo_pose_ws.xgs_f16 = 1), three bf16 pieces otherwise */
int lemo_lbs_verts_fwd_xs(const lemo_skin_const* c, const float* Xg, const unsigned short* XgS, int Bp, const float* A, int nj,
                          const float* transl, const int* ids, int n, int B, float* verts, float* v_posed, void* stream);
int lemo_lbs_verts_fwd_census(const lemo_skin_const* c, const float* Xg, int Bp, const float* A, int nj, const float* transl,
                              int n, int B, float* verts, float* v_posed, unsigned long long* dbg, void* stream,
                              const unsigned short* XgS /* optional, see lemo_lbs_verts_fwd_xs */);
/* forward over a small vertex set U only: verts / v_posed [B][u->n][3] in U's order, identical arithmetic
 * per vertex up to the summation order of the blend GEMM; blend: [B][u->NCs] floats of scratch; needs u->DkT */
int lemo_lbs_verts_fwd_active(const lemo_skin_const* c, const lemo_vertex_set_bwd* u, const float* Xg, int Bp, const float* A,
                              int nj, const float* transl, int B, float* blend, float* verts, float* v_posed, void* stream);
int lemo_lbs_verts_bwd(const lemo_skin_const* c, const lemo_vertex_set_bwd* u, const float* A, int nj, const float* v_posed,
                       int vp_rows, const float* dverts, int B, int Bp, float* dvp, float* dA, float* dtransl, float* dX,
                       void* stream);
int lemo_joints_assemble(const float* Jtr, int nj, const float* verts, int vrows, const int* extra_rows, int n_extra,
                         const int* lmk_rows, const float* lmk_bary, int n_lmk, const float* transl, int B, float* joints,
                         void* stream);

/* ---- marker-image decode / encode around the loop, one clip (T <= 256 frames) per call ----
 * utils/utils.py:184-203 reconstruct_global_body: in [T][J+2][3] = (ignored reference slot, J local joints, trajectory
 * (dx, dz, dr)); rot_0_pivot from the encode below; out [T][J][3] global positions. */
int lemo_reconstruct_global_body(const float* in, int T, int J, double rot_0_pivot, float* out, void* stream);
/* same, rot_0_pivot read from device memory ([1] double, as lemo_local_markers_4chan leaves it): no host round trip */
int lemo_reconstruct_global_body_dev(const float* in, int T, int J, const double* rot_0_pivot, float* out, void* stream);
/* opt_amass_temp.py:273-325 (twin fitting_temp_slide.py:895-940): decode of the infilling network's output in one launch.
 * rec [d][T] = channel 0 of the un-padded output (d = 3 J + 4: J = pelvis + markers rows, then 4 contact logits);
 * traj [3][T] = row 0 of channels 1..3 of the input image (normalised dx, dz, dr); stats [2 d + 4] doubles =
 * Xmean_local[d], Xstd_local[d], Xmean_global_xy, Xstd_global_xy, Xmean_global_r, Xstd_global_r
 * (preprocess_stats_infill_local_markers_4chan.npz); rot_0_pivot [1] double on the device; post [13] floats or NULL =
 * (z shift, M[9] row-major, t[3]): out = (p + (0,0,shift)) . M + t  (PROX: back to the scene frame, :934-939).
 * -> contact_lbl [T][4] in {0,1} (sigmoid > 0.5), markers [T][J-1][3] global (pelvis row dropped). */
int lemo_decode_clip(const float* rec, const float* traj, const double* stats, const double* rot_0_pivot, const float* post, int T,
                     int J, float* contact_lbl, float* markers, void* stream);
/* utils/utils.py:209-265 get_local_markers_4chan: body [T][1+67][3] global pelvis + markers, contact [T][4] ->
 * image [4][T-1][3*68+4] (local markers + contacts | dx | dz | dr repeated) and rot_0_pivot[1] (float64, device). */
int lemo_local_markers_4chan(const float* body, const float* contact, int T, int M1, float* image, double* rot_0_pivot,
                             void* stream);

/* ---- clip images of the two priors from the markers of N clips (dataset_kernels.hip): what loader/train_loader_infill.py:134-330
 * (mode 4CHAN) and loader/train_loader_smooth.py:130-204 (mode SMOOTH) do per clip on the host -- first-frame canonicalisation,
 * contact labels, heading-normalised local representation, dataset statistics, normalisation.  One workgroup per clip;
 * 2 <= T <= 256, 61 <= M <= 83 (LEMO_ERR_SHAPE otherwise).  d = 3 (M + 1) + 4 rows and F = T - 1 frames (4CHAN), d = 3 (M + 1)
 * and F = T (SMOOTH).  fp32 through canonicalisation, labels and floor shift, float64 from there on, one rounding to fp32. */
#define LEMO_CLIP_4CHAN 0
#define LEMO_CLIP_SMOOTH 1
#define LEMO_CLIP_GLOBAL 2   /* train_loader_smooth.py mode global_markers: d = 3 M rows (M = 67 or 81; LEMO_ERR_SHAPE otherwise), F = T,
                              * every row (p - marker 0 of frame 0) . R0 in fp32, all rows normalised, one scalar std */
typedef struct lemo_clip_repr_desc {
  const float* markers;      /* [N][T][M][3] world frame */
  const float* pelvis;       /* [N][T][3] joint 0 */
  const float* hips0;        /* [N][2][3] joints 1 and 2 of frame 0 */
  int n_clips, T, M, mode;
  float fps;                 /* of the clips (contact speed threshold 0.22 m/s) */
  int api_layout;            /* 0: image [N][C][d][F] (what the trainers' upload_dataset takes); 1: [N][C][F][d] (get_local_markers_4chan) */
  const double* stats;       /* [2 d + 4] as lemo_decode_clip reads them, or NULL: unnormalised image.  SMOOTH: mean[d], std[d] (rows
                                0-2 carry their own std and are the only ones normalised), std of all, std of rows 0-2, 0, 0 */
  float* image;              /* write pass; C = 4 (4CHAN) or 1 (SMOOTH, GLOBAL) */
  double* rot_0_pivot;       /* [N] or NULL (4CHAN) */
  float* contact;            /* [N][T][4] in {0, 1} or NULL (4CHAN, write pass) */
  double* stats_part;        /* statistics pass: [N][lemo_clip_repr_stats_k()] per-clip partial sums */
} lemo_clip_repr_desc;
int lemo_clip_repr_stats_k(int M, int mode);
/* per-clip partial sums of the unnormalised representation (d->stats is ignored) */
int lemo_clip_repr_stats(const lemo_clip_repr_desc* d, void* stream);
/* adds the partials of ALL n_clips clips in clip order (one workgroup; no atomics: the result does not depend on how the
 * clips were split into lemo_clip_repr_stats launches) -> stats [2 d + 4], population standard deviations */
int lemo_clip_repr_stats_reduce(const double* stats_part, int n_clips, int T, int M, int mode, double* stats, void* stream);
/* recomputes the representation, normalises in float64 (d->stats) and stores the fp32 image, rot_0_pivot and contact */
int lemo_clip_repr_write(const lemo_clip_repr_desc* d, void* stream);

/* ---- motion-infilling autoencoder, models/AE.py:11-108 and its finetune step, opt_amass_temp.py:154-214 ----
 * (stride-1 convs / transposed convs run on lemo_conv3x3_mfma; these are the remaining layer types) */
/* MaxPool2d(3,2,1): out is CG8P of ((H-1)/2+1) x ((W-1)/2+1); idx [C/8][Ho*Wo][8] winning tap (uint8) */
int lemo_maxpool3s2_fwd(const float* in, int H, int W, float* out, unsigned char* idx, int C, void* stream);
/* din = scatter of dout to the argmax positions (gather form), optionally times lrelu'(act) */
int lemo_maxpool3s2_bwd(const float* dout, const unsigned char* idx, const float* act, float* din, int H, int W, int C, void* stream);
/* zero-stuffing of ConvTranspose2d(stride 2, output_size = H x W): out[2i][2j] = in[i][j]; and its adjoint */
int lemo_stuff2_fwd(const float* in, int h, int w, float* out, int H, int W, int C, void* stream);
int lemo_stuff2_bwd(const float* dout, int H, int W, const float* act, float* din, int h, int w, int C, void* stream);
/* dW[co][ci][3][3] = sum_p dY[co][p] X[ci][p+tap] (+ db[co] = sum_p dY) ; partial: [nslab][9][cout][cin] scratch */
int lemo_conv3x3_wgrad_nslab(int H, int W);
int lemo_conv3x3_wgrad(const float* dy, const float* x, int H, int W, int cin, int cout, int cin_real, int cout_real,
                       float* partial, float* dw, float* db, void* stream);
/* the same in two stages for a whole network: slab partials per layer (any stream), then ONE launch that reduces the partials
   of up to LEMO_WGRAD_MAX_JOBS layers (same summation order as lemo_conv3x3_wgrad: identical bits).  models/AE.py:36-108 has
   20 convolutions; the per-layer reduce launches were 0.25 ms of its 2 ms training step. */
#define LEMO_WGRAD_MAX_JOBS 24
typedef struct lemo_wgrad_job {
  const float* partial;     /* [nslab][9][cout][cin] written by lemo_conv3x3_wgrad_partial */
  const float* dy;          /* CG8P, cout channels (bias gradient) */
  float* dw;                /* [cout_real][cin_real][3][3] */
  float* db;                /* [cout_real] or NULL */
  int nslab, cin, cout, cin_real, cout_real, H, W;
} lemo_wgrad_job;
int lemo_conv3x3_wgrad_partial(const float* dy, const float* x, int H, int W, int cin, int cout, float* partial, void* stream);
int lemo_conv3x3_wgrad_reduce_multi(const lemo_wgrad_job* jobs, int n, void* stream);
/* torch.optim.Adam (defaults) over a flat buffer; step is 1-based */
int lemo_adam_flat(float* p, const float* g, float* m, float* v, int n, float lr, int step, void* stream);
/* same with the step count on the device (step_ctr[0] = completed steps; advanced by one after the update), so that a
 * captured graph of a whole training step can be replayed */
int lemo_adam_flat_ctr(float* p, const float* g, float* m, float* v, int n, float lr, int* step_ctr, void* stream);

/* ---- native training-step engine of the infilling autoencoder (lemo_amd/csrc/ae_engine.hip) ------------------------
 * Replaces, for one clip, the block opt_amass_temp.py:160-214 (= temp_prox/fitting_temp_slide.py:861-893): "reload the
 * pretrained AE, optimizer = Adam(lr 3e-6), 60 x [rec = AE(x); loss = sum(|rec - x| * mask) / count; backward; step],
 * eval forward".  One step is 53 launches (20 + 19 convolutions with fused epilogues, pooling, ONE launch for all 20 weight
 * gradients, ONE for slab reduction + Adam + re-packing), captured into 5-step and 1-step graphs on first use.
 *   ws / ws_floats: caller-owned ZEROED device workspace of lemo_ae_ws_floats(H, W) floats, alive as long as the engine;
 *   H x W: the clip image [1,4,H,W] (H = 3 * markers + contacts + 2 pads, W = frames + 16), H, W >= 2, H * W <= 2^22.
 * lemo_ae_load: `flat` = the model's 40 tensors back to back in state_dict order per layer (weight, bias; enc_blc1.main.0,
 *   enc_blc1.main.2, ..., dec_blc5.deconv2; each in its own layout: Conv2d [out][in][3][3], ConvTranspose2d [in][out][3][3]),
 *   lemo_ae_n_param() floats; x = clip image [4][H][W]; moc = train mask / count, [H][W] (d loss / d rec = sign(rec - x) * moc).
 *   Resets the optimizer state (a fresh Adam per clip, as the reference builds one).
 * lemo_ae_step: n training steps on `stream` (use_graph: replay captured steps; same kernels, same results).
 * lemo_ae_forward: eval forward with the current parameters -> rec [H][W], z [256][h5][w5] (may be NULL; h5, w5 = five times
 *   (n - 1) / 2 + 1).   lemo_ae_params: the current parameters in `flat` order. */
typedef struct lemo_ae_desc {
  int H, W;
  float lr;
  float* ws;
  long long ws_floats;
  int clips;                      /* round 4 (appended; 0 or 1 = one clip): K clips SIDE BY SIDE in every launch of a step -- the clip is
                                   * the last grid dimension of the convolution / pooling / weight-gradient / Adam launches, each clip has
                                   * its own parameters, Adam state and step counter in its own slice of the workspace (the reference
                                   * finetunes a fresh copy of the pretrained model per clip): ws_floats >= clips * lemo_ae_ws_floats(H, W).
                                   * Round 5: the convolutions' launch shapes are chosen for the clips in flight (18.0 -> 16.4 ms per clip at
                                   * 8): a clip's results depend on `clips` through the order its K slices are summed in -- bit-identical
                                   * for equal `clips` and between the slots of one engine, equal to a one-clip engine's to rounding. */
} lemo_ae_desc;
long long lemo_ae_ws_floats(int H, int W);
int lemo_ae_n_param(void);
void* lemo_ae_create(const lemo_ae_desc* d);
void lemo_ae_destroy(void* h);
int lemo_ae_load(void* h, const float* flat, const float* x, const float* moc, void* stream);
int lemo_ae_step(void* h, int n, int use_graph, void* stream);          /* every clip of the engine advances n steps */
int lemo_ae_forward(void* h, float* rec, float* z, void* stream);
int lemo_ae_params(void* h, float* flat_out, void* stream);
/* the same per clip of a multi-clip engine (clip 0 .. desc.clips - 1; the un-suffixed forms address clip 0).  lemo_ae_forward_clip with
 * clip 0 (or -1: no copy-out) runs the eval forward of ALL clips; clips > 0 only copy that forward's reconstruction / latent out:
 * call it for clip 0 first.  State rules (LEMO_ERR_STATE otherwise): lemo_ae_step / lemo_ae_forward* need EVERY clip of the engine loaded
 * since creation (a step advances all of them; an unloaded clip would train from a zeroed workspace); lemo_ae_forward_clip(clip > 0) needs
 * an eval forward (clip 0 or -1) AFTER the last step / load; lemo_ae_params_clip needs that clip loaded. */
int lemo_ae_load_clip(void* h, int clip, const float* flat, const float* x, const float* moc, void* stream);
int lemo_ae_forward_clip(void* h, int clip, float* rec, float* z, void* stream);
int lemo_ae_params_clip(void* h, int clip, float* flat_out, void* stream);
/* diagnostics (tools/ae_wgrad_probe.py): the step's weight-gradient launch alone on the engine's current buffers; mode 0 = as in
 * a step, 1 = operands loaded once per wave, 2 = loads without MFMAs (1 and 2 leave garbage in the slab partials). */
int lemo_ae_wgrad_probe(void* h, int mode, void* stream);
/* one convolution of the engine on its own (tests, tools).  Enumerates an H x W pixel grid; in_s = 2: the input (and the
 * epi-1 operand) is a fineH x fineW image read at its even pixels; out_s = 2: the output is written to the even pixels of a
 * fineH x fineW image (zero-stuffing geometry).  mt = 0: the engine's own launch shape; else tile mt (1: 32 px x 32 cout,
 * 2: 32 x 64, 3: 16 x 16) with pt pixel tiles x ks K-slices = pt * ks <= 16 waves per workgroup. */
int lemo_ae_conv(const float* in, const float* wt, const float* bias, const float* aux, float* out, int H, int W, int fineH, int fineW,
                 int in_s, int out_s, int cin, int cout, int epi, int mt, int pt, int ks, void* stream);
/* ... on the split-f16 kernels (round 6, the engine's default arithmetic): both operands are read as fp32 and split in registers into two
 * error-compensated fp16 pieces, three f16 MFMA products, fp32 accumulate.  amax_in [1] = max |in| (or a bound, multiplied by in_fac >= 1),
 * wmax [1] = max |wt|, amax_out [1] receives max |out| of the launch (atomicMax: zero it first).  cin >= 16 (mt 3: cin >= 32). */
int lemo_ae_conv_f16(const float* in, const float* wt, const float* bias, const float* aux, float* out, int H, int W, int fineH, int fineW,
                     int in_s, int out_s, int cin, int cout, int epi, int mt, int pt, int ks, const float* amax_in, float in_fac,
                     const float* wmax, float* amax_out, void* stream);

/* ---- smoothness-prior training: models/AE_sep.py Enc + Dec (downsample=False, z_channel=64), train_smooth_prior.py:96-136 ----
 * One step on a batch of network inputs x [bs][H][W] (the reflect-padded velocity image, 245 x 135 for T = 120, 81 markers):
 *   z = Enc(x), rec = Dec(z), loss = weight_rec * mean|x - rec| + weight_smooth * mean((z[..., 1:] - z[..., :-1])^2),
 *   torch.optim.Adam(lr) with default betas / eps over all 40 tensors.  fp32 throughout, every sum in a fixed order: two engines
 *   (and a graph replay and an eager run) give identical bits.  Forward / backward-data of the 32- and 64-channel layers run on
 *   lemo_conv3x3_mfma_lds, one launch per image and layer; the weight gradients on lemo_wgrad3x3_batched's kernels.
 *   ws / ws_floats: caller-owned ZEROED device workspace of lemo_sptrain_ws_floats(H, W, bs) floats (0: a shape the kernels do not take:
 *   2 <= H, 2 <= W <= 139), alive as long as the engine.  use_graph: capture the step once, replay it (same kernels, same bits).
 * lemo_sptrain_load: flat = lemo_sptrain_n_param() floats (device), the 20 Enc tensors then the 20 Dec tensors in state_dict order
 *   (enc_blcN.main.{0,2}.{weight,bias}: Conv2d [out][in][3][3]; dec_blcN.deconv{1,2}.{weight,bias}: ConvTranspose2d [in][out][3][3]);
 *   resets the optimizer.  Step / eval / params / grads before a load: LEMO_ERR_STATE.
 * lemo_sptrain_step: n steps on x; losses (device, may be NULL) <- {L1 term, smoothness term, weighted total} of the last step.
 * lemo_sptrain_eval: the same losses under the current parameters, no update; rec (may be NULL) <- [bs][H+2][W+2] (zero border).
 * lemo_sptrain_params / _grads: the parameters / the last step's gradient in `flat` order. */
typedef struct lemo_sptrain_desc {
  int H, W, bs;
  float lr;
  float weight_rec, weight_smooth;      /* train_smooth_prior.py defaults: 1.0, 1000.0 */
  float* ws;
  long long ws_floats;
  int use_graph;
} lemo_sptrain_desc;
long long lemo_sptrain_ws_floats(int H, int W, int bs);
int lemo_sptrain_n_param(void);
void* lemo_sptrain_create(const lemo_sptrain_desc* d);
void lemo_sptrain_destroy(void* h);
int lemo_sptrain_load(void* h, const float* flat, void* stream);
int lemo_sptrain_step(void* h, const float* x, int n, float* losses, void* stream);
int lemo_sptrain_eval(void* h, const float* x, float* losses, float* rec, void* stream);
int lemo_sptrain_params(void* h, float* flat_out, void* stream);
int lemo_sptrain_grads(void* h, float* flat_out, void* stream);
/* batched 3x3 weight gradient: gw[m][n][ky][kx] = sum_{b,y,x} A_b[m][y][x] B_b[n][y+ky-1][x+kx-1], gb = per-channel sums of B
 * (bias_b) or A.  ca, cb in {32, 64}: CG8P operands, fp32 MFMA; cb == 1 with ca in {1, 32}: the 1-channel operands are plain padded
 * images [(H+2)(W+2)], FMA kernel.  Image b's operand starts a_stride / b_stride floats after image b-1's.  ws: device scratch of
 * lemo_wgrad3x3_batched_ws_floats() floats.  LEMO_ERR_SHAPE for channel counts it does not take or W > 157 (MFMA form). */
long long lemo_wgrad3x3_batched_ws_floats(int H, int W, int bs, int ca, int cb);
int lemo_wgrad3x3_batched(const float* A, long long a_stride, const float* B, long long b_stride, int bs, int H, int W, int ca, int cb,
                          int bias_b, float* ws, float* gw, float* gb, void* stream);
/* Dec's last block, dec_blc5 (models/AE_sep.py DecBlock_output, stride 1): r1 = lrelu(deconv_{32->1}(u) + b8), rec = deconv_{1->1}(r1)
 * + b9.  u: 32-channel CG8P per image (u_stride floats apart); w8 [32][1][3][3], w9 [1][1][3][3]; r1, rec: [bs][H+2][W+2], border
 * left as the caller zeroed it. */
int lemo_dec_end_fwd(const float* u, long long u_stride, const float* w8, const float* b8, const float* w9, const float* b9, float* r1,
                     float* rec, int bs, int H, int W, void* stream);

/* ---- infilling-prior training: models/AE.py AE(downsample=True, in_channel=4, kernel=3), train_infill_prior.py:185-203
 * (lemo_amd/csrc/ae_train_engine.hip).  One step on a batch of bs images with ONE parameter set:
 *   x [bs][4][H][W]: the masked, reflect-padded network input; y [bs][H][W]: the unmasked padded target (channel 0); rec = AE(x);
 *   L_body = mean |y - rec| over rows r < H - 5, L_v = mean |dy - drec| over the same rows and the W - 1 column differences,
 *   L_c = BCEWithLogits(rec, y) over the 5 bottom rows; total = w_body L_body + w_v L_v + w_c L_c (train_infill_prior.py defaults
 *   10, 10, 1); torch.optim.Adam(lr) with default betas / eps over all 40 tensors.  fp32 (fp32-input MFMA), every sum in a fixed
 *   order: a graph replay, an eager run and a second engine give identical bits.
 *   Shapes: 1 <= bs <= 128, H >= 6, W >= 2, H W <= 2^22 (lemo_aetrain_ws_floats returns 0 otherwise).  ws / ws_floats: caller-owned
 *   ZEROED device workspace of lemo_aetrain_ws_floats(H, W, bs) floats, alive as long as the engine.  use_graph: capture the step
 *   once, replay it.
 * lemo_aetrain_load: flat = lemo_ae_n_param() floats (device) in lemo_ae_load's order; resets the optimizer.  Step / eval / params /
 *   grads before a load: LEMO_ERR_STATE.
 * lemo_aetrain_step: n >= 1 steps on (x, y); losses (device, may be NULL) <- {L_body, L_v, L_c, total} of the last step.
 * lemo_aetrain_eval: the same losses under the current parameters, no update; rec (device, may be NULL) <- [bs][H][W].
 * lemo_aetrain_params / _grads: the parameters / the last step's gradient (summed over the batch) in `flat` order.
 * lemo_aetrain_pool_winners: the max-pool winners of encoder block `block` (0 .. 4) in the last forward, out (device) <- bs x
 *   [C/8][Ho][Wo][8] bytes (C = the block's channels, Ho, Wo its pooled size), each the winning tap ky * 3 + kx of the 3 x 3 window
 *   (first maximum in row-major order, as torch).  The max-pool adjoint routes every gradient through these. */
typedef struct lemo_aetrain_desc {
  int H, W, bs;
  float lr;
  float w_body, w_v, w_c;
  float* ws;
  long long ws_floats;
  int use_graph;
} lemo_aetrain_desc;
long long lemo_aetrain_ws_floats(int H, int W, int bs);
void* lemo_aetrain_create(const lemo_aetrain_desc* d);
void lemo_aetrain_destroy(void* h);
int lemo_aetrain_load(void* h, const float* flat, void* stream);
int lemo_aetrain_step(void* h, const float* x, const float* y, int n, float* losses, void* stream);
int lemo_aetrain_eval(void* h, const float* x, const float* y, float* losses, float* rec, void* stream);
int lemo_aetrain_params(void* h, float* flat_out, void* stream);
int lemo_aetrain_grads(void* h, float* flat_out, void* stream);
int lemo_aetrain_pool_winners(void* h, int block, unsigned char* out, void* stream);

/* ---- the loop level of both training engines: a whole epoch of DIFFERENT batches with the dataset on the device
 * (lemo_amd/csrc/train_epoch_kernels.hip).  For s = 0 .. n_steps - 1: one kernel assembles batch s from the device-resident clips
 * straight into the engine's staging buffers, the engine runs one step (train != 0) or forward + losses (train == 0: the
 * reference's test-loss loop; the caller averages), and the step's losses go to row s of `log` (device, caller-owned: AE
 * {L_body, L_v, L_c, total}, smoothness {L1, smooth, total}).  The host never waits between steps; with use_graph ONE captured
 * chain (assemble, step, log) is replayed n_steps times: the step cursor lives in device memory.  Same kernels and bits as
 * n_steps lemo_*train_step calls on the same batches.
 * Infilling prior: data [n_clips][4][H-2][W-16] (the unpadded clip images), idx [n_steps][bs] int32.  Batch s is
 *   x = reflect_pad(mask(clip), (8, 8, 1, 1)), y = reflect_pad(clip)[:, 0]; the mask (channel 0 only, before the padding) is
 *   LEMO_MASK_NONE:   none (input = target);
 *   LEMO_MASK_RANDOM: marker_ids [n_steps][bs][6] int32 in -1 .. 66 (-1: unused slot): rows 3 + 3 id .. + 2 set to 0; rows d-4 and
 *                     d-2 if 16 or 30 is among the slot's ids, rows d-3 and d-1 if 47 or 60 is (train_infill_prior.py:135-160);
 *   LEMO_MASK_PROX:   masks [n_masks][67][mask_len] fp32 (marker-major, frame fastest; mask_len >= W - 16, frames 0 .. W-17 are
 *                     used), mask_idx [n_steps][bs] int32: the 3 pelvis rows x 1, each marker's 3 rows x its mask, the contact
 *                     rows x (both markers of that foot == 1) (train_infill_prior.py:162-178).
 *   The masking recipes need H - 2 == 208 (67 markers).  W >= 25.
 * Smoothness prior: data [n_clips][1][H-2][W-15]; batch s is reflect_pad(clip[..., 1:] - clip[..., :-1], (8, 8, 1, 1)).  W >= 25, H >= 4.
 * Every index is the CALLER's to validate (0 <= idx < n_clips, -1 <= id < 67, 0 <= mask_idx < n_masks): the tables live on the
 * device (the kernels clamp clip and mask indices into range so that a bad table cannot read outside the buffers).
 * LEMO_ERR_ARG: null pointers, counts < 1, a shape that does not fit the recipe; LEMO_ERR_STATE: _epoch before a load.
 * lemo_*train_batch: batch `step` of the same descriptor in the API layout (x [bs][4][H][W], y [bs][H][W]; smoothness x [bs][H][W])
 *   through the same device function, for inspection and tests (`log`, `train` unused).
 * Training state: lemo_*train_state_floats() = 3 P + 2 floats (P = lemo_ae_n_param() / lemo_sptrain_n_param()), one fp32 blob:
 *   [0, P) parameters, [P, 2P) Adam's first moments, [2P, 3P) second moments, each in the engine's `flat` order;
 *   [3P] = step mod 2^24, [3P + 1] = step div 2^24 (Adam's step counter, both exact in fp32).
 *   _state_load rebuilds every pack _load rebuilds and does NOT reset the optimizer: the engine continues bit-identically. */
#define LEMO_MASK_NONE 0
#define LEMO_MASK_RANDOM 1
#define LEMO_MASK_PROX 2
typedef struct lemo_aetrain_epoch_desc {
  const float* data;
  int n_clips;
  const int* idx;
  int n_steps;
  int recipe;
  const int* marker_ids;
  const float* masks;
  int n_masks, mask_len;
  const int* mask_idx;
  float* log;
  int train;
} lemo_aetrain_epoch_desc;
typedef struct lemo_sptrain_epoch_desc {
  const float* data;
  int n_clips;
  const int* idx;
  int n_steps;
  float* log;
  int train;
} lemo_sptrain_epoch_desc;
int lemo_aetrain_epoch(void* h, const lemo_aetrain_epoch_desc* d, void* stream);
int lemo_aetrain_batch(void* h, const lemo_aetrain_epoch_desc* d, int step, float* x, float* y, void* stream);
long long lemo_aetrain_state_floats(void);
int lemo_aetrain_state_save(void* h, float* out, void* stream);
int lemo_aetrain_state_load(void* h, const float* in, void* stream);
int lemo_sptrain_epoch(void* h, const lemo_sptrain_epoch_desc* d, void* stream);
int lemo_sptrain_batch(void* h, const lemo_sptrain_epoch_desc* d, int step, float* x, void* stream);
long long lemo_sptrain_state_floats(void);
int lemo_sptrain_state_save(void* h, float* out, void* stream);
int lemo_sptrain_state_load(void* h, const float* in, void* stream);

/* ---- stream capture helpers: record everything a host-side step enqueues on `stream` (HIP kernels of this library
 * and the caller's own device work alike) into an executable graph, replay it with one call.  Relaxed capture mode;
 * the caller guarantees that the step does not synchronise and that every buffer it touches outlives the replays. */
int lemo_capture_begin(void* stream);
int lemo_capture_end(void* stream, void** graph_exec);
int lemo_graph_launch(void* graph_exec, void* stream);
int lemo_graph_destroy(void* graph_exec);

/* ---- PROX scene terms: F.grid_sample(sdf, verts, padding_mode='border') of temp_prox/fitting_temp_slide.py:685-739
 * sdf [D][H][W] device; pts [N][3] device world coordinates; gmin/gmax HOST float[3]; val [N]; dval [N][3] or NULL
 * (d val / d pts).  Grid axis order follows the reference's norm_vertices[:, :, [2,1,0]]. */
int lemo_sdf_sample(const float* sdf, int D, int H, int W, const float* pts, int N, const float* gmin, const float* gmax,
                    float* val, float* dval, void* stream);

/* ---- AMASS temporal fitting iteration, opt_amass_temp.py:349-455 -------------------------------- */
typedef struct lemo_fit_const {
  int n, n67, n81;
  const int *row67, *row81, *foot_start, *foot_row, *u_row, *u_m67, *u_m81, *u_foot_mask;
  const float *Xstd, *Xmean;
  const float* cam2world;         /* optional [12] = R row-major, t (PROX, fitting_temp_slide.py:676-680): the canonical frame
                                   * is built from WORLD joints R (J + transl) + t and applied to world markers R v + t; the
                                   * published canon matrix is R^T R0 so that it acts on camera-frame vertices directly */
} lemo_fit_const;

/* conv variant 7 (round 5) = variant 5 + the encoder's head and tail as ONE launch each (csrc/conv_head_kernels.hip):
 *   lemo_enc_head: canonicalised marker image (opt_amass_temp.py:366-392) -> layer 0 (1 -> 32, fp32 FMAs, bit-identical to lemo_conv3x3_c1 on the
 *     published x0) -> layer 1 (32 -> 32, split-f16 MFMA; w1pack / w1inv = pack_conv3x3_split_f16 of its weights) -- writes x0 (padded image),
 *     canon [12], act1 and act2 (CG8P, 32 channels each); replaces the marker_c1 launch + one single-layer launch;
 *   lemo_enc_tail: d(pre-act 2) (CG8P, 32 channels) -> layer 1 backward-data x lrelu'(act1) (w1bpack = pack_conv3x3_bwd_split_f16) -> layer 0
 *     adjoint (w0 [32][9]) -> dx0 [H * W]; replaces one single-layer launch + lemo_conv3x3_c1_bwd; d(pre-act 1) stays in LDS. */
int lemo_enc_head(const lemo_fit_const* fc, const float* verts, int nrows, const float* Jtr, int nj, const float* transl, int B, const float* w0,
                  const float* b0, const void* w1pack, float w1inv, const float* b1, float* x0, float* canon, float* act1, float* act2,
                  void* stream);
int lemo_enc_tail(const float* din, const void* w1bpack, float w1binv, const float* act1, const float* w0, float* dx0, int H, int W,
                  void* stream);
/* conv variant 9: the tail with layer 2's backward-data in front -- d(pre-act 3) (CG8P, 64 channels) -> conv^T 64 -> 32 x lrelu'(act2)
 * (w2bpack = pack_conv3x3_bwd_split_f16 of layer 2) -> lemo_enc_tail's two stages -> dx0; replaces two single-layer launches +
 * lemo_conv3x3_c1_bwd (models/AE_sep.py:16-21 backwards); d(pre-act 2) and d(pre-act 1) stay in LDS. */
int lemo_enc_tail3(const float* din, const void* w2bpack, float w2binv, const float* act2, const void* w1bpack, float w1binv, const float* act1,
                   const float* w0, float* dx0, int H, int W, void* stream);

typedef struct lemo_fit_desc {
  int B, Bp, V, nrows;            /* frames, padded frames, model vertices, rows of `verts` (V or n) */
  int full_vertices;              /* 1: regress all V vertices per frame (reference behaviour) ; 0: only the set U */
  int conv_variant;               /* kernel family of the encoder's MFMA layers (the struct has no default: 0 selects lemo_conv3x3_mfma variant 0;
                                   * lemo_amd.priors.DEFAULT_CONV_VARIANT = 9 is what the Python fitters pass and what every gate runs on):
                                   * 9 (shipped): lemo_enc_head3 (image + layers 0-2) + fused 64 -> 64 pairs (lemo_conv3x3_pair_f16) + lemo_enc_tail3
                                   *    (layers 2-0 backwards), split-f16 arithmetic throughout; lemo_fit_step runs layer 9, the smoothness loss and
                                   *    layer 9's backward as ONE launch (lemo_conv3x3_turn_f16; the environment variable LEMO_ENC_TURN=0, read by
                                   *    lemo_fit_create, keeps the three launches) ; 8: 9 with layer 2's backward a launch of its own ;
                                   * 7: head / tail without layer 2 (lemo_enc_head / lemo_enc_tail) ; 5: pairs only, head and tail layer by layer ;
                                   * 10 (round 6): 9 with every 64 -> 64 layer ONE Winograd launch (lemo_conv3x3_wino_f16) instead of the pairs --
                                   *    parity-green, measured slower, enc_w3 / enc_wbwd3 of those layers then hold the Winograd packs ;
                                   * 4: split-f16, one launch per layer ; 3: split-bf16 (lemo_conv3x3_mfma_split) where it takes the shape, else 2 ;
                                   * 2: lemo_conv3x3_mfma_lds ; 0 / 1: lemo_conv3x3_mfma variants (the any-shape fallback of all the others).
                                   * (6, the pairs on four-wave workgroups, left the library in round 6: csrc/attic) */
  lemo_vposer_w vposer;
  lemo_body_const body;
  lemo_skin_const skin;
  lemo_vertex_set_bwd uset;
  lemo_fit_const fit;
  const int* fwd_ids;             /* [n] when !full_vertices */
  /* smoothness encoder: 10 layers; channels ch[0..10] = 1,32,32,64,... */
  int enc_ch[11];
  const float* enc_w[10];         /* layer 0: [Cout][9] ; others packed wt[tap][Cin/8][Cout][8] */
  const float* enc_b[10];
  const float* enc_wbwd[10];      /* backward-data packs (layer 0: same [Cout][9]) */
  const float* enc_w2[10];        /* channel-group-major packs for conv_variant 2 (layer 0 unused) */
  const float* enc_wbwd2[10];
  const void* enc_w3[10];         /* split packs (layer 0: NULL): bf16 x 3 pieces for conv_variant 3, f16 x 2 pieces for 4 */
  const void* enc_wbwd3[10];
  float enc_w3_inv[10];           /* conv_variant 4: 2^-k of each pack's host-side weight scale 2^k (lemo_conv3x3_mfma_split_f16) */
  float enc_wbwd3_inv[10];
  /* sequence data */
  const float* target;            /* [B][n67][3]  markers_rec */
  const float* contact;           /* [B][4] */
  const float* weights;           /* [6] rec_markers, vposer, shape, hand, contact_vel, smooth (device) */
  float weights_host[6];          /* same values, host copy (launch-time constants) */
  /* optimised parameters + Adam state */
  float *transl, *rot6d, *other;  /* [B][3], [B][6], [B][56] */
  const float* shape;             /* [B][10] fixed */
  float *adam_m[3], *adam_v[3];
  int* step_ctr;
  float lr0, lr1;
  int lr_switch;
  /* workspace (caller-allocated, sizes documented in lemo_amd/fitting.py) */
  float *go_aa, *body_aa, *h1, *h2, *vo, *vp_scratch;   /* vp_scratch [B][1152] */
  lemo_pose_ws pose;
  float *verts, *v_posed, *x0, *canon;
  float* act[11];                 /* act[0] unused; act[l] = output of layer l, CG8P */
  float* dact[2];                 /* ping-pong d(pre-activation) buffers, 64-channel CG8P */
  float *dx0, *spartial, *vpartial, *losses, *dverts, *dvp, *dA, *dX;
  double* loss_acc;               /* [32][16] per-iteration loss accumulators (f64 atomics, 32 slots) */
  int* step_cur;                  /* [1] step index latched at the start of the iteration */
  float *g_transl, *g_rot6d, *g_other, *g_go, *g_body;
  /* ---- round-2 additions (appended: earlier offsets unchanged; all optional / zero = previous behaviour) ---- */
  float* snap;                    /* [B*65] or NULL: every Adam update first stores the PRE-update parameters here
                                   * (transl [B][3] | rot6d [B][6] | other [B][56]): with go_aa of the same iteration's
                                   * forward this is the reference's body_params_opt_t_72 (opt_amass_temp.py:457) */
  int* nonfinite;                 /* [2] or NULL, zeroed by the caller.  [0]: 1-based index of the first iteration whose
                                   * total loss was NaN / Inf (0 = none), written by the Adam kernel; [1]: its copy latched at
                                   * the start of the next iteration.  Once latched, parameter updates are skipped: the device
                                   * side of FittingMonitor.run_fitting's "NaN/Inf loss -> stop" (fitting_temp_slide.py:198-204);
                                   * like there, the update of the offending iteration itself has already been applied. */
  int per_frame;                  /* 1: opt_amass_perframe.py:324-351 -- marker L1 + the three L2 priors only (no smoothness
                                   * encoder, no contact term), any B >= 1 */
  float lr2;                      /* third learning-rate level: lr = lr2 when step > lr_switch2 > 0 (opt_amass_perframe.py:316-321) */
  int lr_switch2;
  /* ---- round-6 addition (appended; NULL = previous behaviour): the all-vertex forward OFF the iteration's critical path ---- */
  float* verts_side;              /* [B][V][3] or NULL.  With full_vertices = 0 (the loss path forwards only the set U): every iteration ALSO regresses
                                   * all V vertices of its pose into this buffer (what the reference's smplx forward returns: utils/utils.py:152), by a
                                   * launch on the engine's own side stream that starts behind the encoder's backward tail and runs beside the per-frame
                                   * launches of the iteration's end (119 of 256 CUs); it is joined before the next iteration's pose stage overwrites its
                                   * operands, and at the end of every call / graph.  Same kernel, same bits as the in-line forward of full_vertices = 1. */
  float* transl_side;             /* [B][3], required with verts_side: the translation of the iteration's forward (the Adam launch updates `transl` while
                                   * the side launch is in flight; the set-U forward leaves a copy here) */
} lemo_fit_desc;

/* Opaque engine: holds a copy of the descriptor (pointers only) and, optionally, a captured hipGraph. */
void* lemo_fit_create(const lemo_fit_desc* d);
void lemo_fit_destroy(void* h);
/* one forward pass only (no backward / Adam): fills verts, losses, ... */
int lemo_fit_forward(void* h, void* stream);
/* after lemo_fit_forward: gradients of the total loss into g_transl / g_rot6d / g_other (priors' own
 * gradient terms are added inside the Adam kernel), no parameter update */
int lemo_fit_backward(void* h, void* stream);
/* n full iterations (forward, backward, Adam).  use_graph: the call is replayed from hipGraphs -- a 1-iteration and a
 * 5-iteration graph to get the device going, then 20-iteration graphs, then ONE graph for what is left (sizes 1 .. 20 are captured on
 * first use, on `stream`, which must not be the legacy default stream, and kept). */
int lemo_fit_step(void* h, int n, int use_graph, void* stream);
/* record (without running anything) the graphs an n-iteration lemo_fit_step(use_graph = 1) on `stream` will replay,
 * so that the first such call does not pay for capture + instantiation */
int lemo_fit_prepare(void* h, int n, void* stream);
/* Diagnostics (bench.py's per-stage figures): average duration in ms of every stage of ONE iteration, each measured as `reps`
 * back-to-back repetitions of the stage's own launches captured into a graph and replayed between two events (consecutive graph
 * nodes, like inside the iteration): ms[0] VPoser decode + pose stage, [1] vertex stage (lbs_verts_fwd), [2] marker image + first
 * layer + encoder forward, [3] losses, [4] encoder backward-data + first-layer adjoint, [5] vertex-stage backward (+ d(verts)),
 * [6] pose / VPoser backward + tail (no update), [7] = LEMO_FIT_NSTAGE: the whole forward + backward the same way.  `stream` must be
 * capturable (not the legacy default stream).  The call SYNCHRONISES (event timing) and leaves losses / gradients of a clean
 * forward + backward of the current parameters behind; parameters and optimiser state are not touched. */
#define LEMO_FIT_NSTAGE 7
int lemo_fit_census(void* h, int reps, float* ms_out /* host [LEMO_FIT_NSTAGE + 1] */, void* stream);
/* Optimiser state of a fit = what torch.optim.Adam + the three parameter tensors hold between two iterations of
 * opt_amass_temp.py:349-455 (opt_amass_perframe.py:312-355 for per_frame engines): the parameters, Adam's exp_avg /
 * exp_avg_sq and the number of completed steps (which also selects the learning-rate level, :350-352).  All pointers are
 * caller-owned DEVICE buffers shaped like the descriptor's ([B][3], [B][6], [B][56] each; step: int[1]).
 * lemo_fit_load_state: engine <- st (and the NaN / Inf latch is cleared): the next lemo_fit_step continues from that state as
 *   if the engine had produced it itself -- used to resume a fit and, in the parity tests, to run ONE step from a state the
 *   reference's own loop went through (teacher forcing) instead of comparing free-running trajectories.
 * lemo_fit_save_state: st <- engine.  One kernel launch each, asynchronous on `stream`, capturable. */
typedef struct lemo_fit_state {
  float *transl, *rot6d, *other;
  float *adam_m[3], *adam_v[3];   /* transl, rot6d, other */
  int* step;                      /* [1] completed Adam steps */
} lemo_fit_state;
int lemo_fit_load_state(void* h, const lemo_fit_state* st, void* stream);
int lemo_fit_save_state(void* h, const lemo_fit_state* st, void* stream);

/* ---- PROX sliding-window fitting iteration (the twin of the loop body above) ------------------------------------------
 * temp_prox/fitting_temp_slide.py: closure fitting_func :239-311 (VPoser decode, SMPL-X, loss, backward, erase of the
 * first int(0.15 B) frames' gradients unless first_batch_flag), SMPLifyLoss.forward as configured by
 * cfg_files/PROXD_temp_S2.yaml / S3.yaml -- 2-D keypoints :573-580 through PerspectiveCamera (camera.py:88-116, fixed
 * identity pose) and JointMapper (misc_utils.py:44-57); L2 / angle priors :586-615 (prior.py:50-90); cam -> world
 * :676-680; SDF penetration :685-694; friction :699-739; infill L1 + contact velocity :944-992 (S3); smoothness prior
 * :997-1031; sum + loss_dict :1036-1061 -- and Adam (optimizers/optim_factory.py:43-46, lr 0.005).  Every .item() branch
 * of the reference is a device-side count; nothing returns to the host. */
typedef struct lemo_prox_const {
  int n_op, n_sj;                 /* OpenPose keypoints (118); smplx joints nj + n_extra + n_lmk (127) */
  const int* joint_map;           /* [n_op] smplx joint each keypoint reads */
  const int *jm_start, *jm_list;  /* inverse of joint_map: CSR [n_sj + 1], [n_op] */
  int n_extra, n_lmk;
  const int* extra_rows;          /* [n_extra] vertex-pick joints */
  const int* lmk_rows;            /* [n_lmk][3] face vertices of the barycentric landmarks */
  const float* lmk_bary;          /* [n_lmk][3] */
  /* S: sorted unique ids of every vertex that carries a term besides the SDF penetration (friction set, 67 + 81 markers,
   * heel / toe sets, vertex-pick joints, landmark face vertices) */
  int n_s;
  const int *s_vid, *s_m67, *s_m81, *s_foot_mask, *s_fric;   /* [n_s]: position in the respective list or -1; 4-bit mask */
  const int *s_jstart, *s_jidx;   /* CSR [n_s + 1] over (vertex-joint index in [0, n_extra + n_lmk), weight) */
  const float* s_jw;
  int n_fric;
  const int* fric_vid;            /* [n_fric] contact_fric_verts_ids (fit_temp_loadprox_slide.py:343-349) */
  int n67;
  const int* m67_vid;             /* [n67] infill markers */
  const int *foot_start, *foot_vid;   /* [5], [...]: left heel, right heel, left toe, right toe */
} lemo_prox_const;

/* weights[13] (device + host copy): data, body_pose, shape, bending_prior, hand_prior, expr_prior, jaw_prior,
 * sdf_penetration, motion_prior_smooth, friction_normal, friction_tangent, motion_infill_rec, motion_infill_contact */
#define LEMO_PROX_NW 13
/* losses[16]: the 14 loss_dict entries in the reference's order (:1047-1061) -- total_loss, joint_loss, s2m_dist, m2s_dist,
 * self_penetration_loss, sdf_penetration_loss, contact_loss, smooth_acc_loss, smooth_vel_loss, motion_prior_smooth_loss,
 * loss_fric_tangent, loss_fric_normal, motion_infill_loss, motion_infill_contact_loss -- then 2 spare */
typedef struct lemo_prox_desc {
  int B, Bp, V;
  int conv_variant;
  int first_batch_flag;           /* 0: gradients of frames [0, int(0.15 B)) are erased every iteration (:282-289) */
  int use_infill;                 /* S3 terms live (marker_mask has an occluded entry, :944) */
  int T;                          /* rows of body_markers_rec / contact_lbl_rec (B - 1) */
  lemo_vposer_w vposer;
  lemo_body_const body;
  lemo_skin_const skin;
  lemo_vertex_set_bwd uset;       /* ALL vertices, with jcsr_chunk + part (deterministic dense backward) */
  lemo_fit_const fit;             /* smoothness-marker tables: n81, row81, Xstd, Xmean, cam2world */
  lemo_prox_const pc;
  int enc_ch[11];
  const float* enc_w[10]; const float* enc_b[10]; const float* enc_wbwd[10];
  const float* enc_w2[10]; const float* enc_wbwd2[10];
  const void* enc_w3[10]; const void* enc_wbwd3[10];
  float enc_w3_inv[10]; float enc_wbwd3_inv[10];      /* conv_variant 4 (see lemo_fit_desc) */
  /* scene */
  const float* sdf; int sdf_dim[3];           /* [D][H][W] */
  float grid_min[3], grid_max[3];
  float cam2world[12];            /* R row-major, t (host copy; fit.cam2world is the device copy) */
  float cam[4];                   /* fx, fy, cx, cy (PROXD_temp_S2.yaml:111-114) */
  /* window data */
  const float* gt_joints;         /* [B][n_op][2] */
  const float* w2;                /* [B][n_op] (joint_weights * joints_conf)^2 */
  const float* marker_mask;       /* [B][n67] or NULL */
  const float* body_markers_rec;  /* [T][n67][3] or NULL */
  const float* contact_lbl_rec;   /* [T][4] or NULL */
  const float* weights;           /* device [LEMO_PROX_NW] */
  float weights_host[LEMO_PROX_NW];
  /* parameters (the smplx module's nn.Parameters + pose_embedding), fixed betas */
  float *global_orient, *transl, *left_hand_pose, *right_hand_pose, *jaw_pose, *leye_pose, *reye_pose, *expression, *pose_embedding;
  const float* betas;             /* [B][10] */
  float *adam_m, *adam_v;         /* [B][81] each, parameter order as listed above */
  int* step_ctr; int* step_cur; int* nonfinite;   /* [1], [1], [2] */
  float lr;
  /* workspace */
  float *h1, *h2, *vo, *vp_scratch;
  lemo_pose_ws pose;
  float *verts, *v_posed, *dverts;            /* [B][V][3] */
  float *x0, *canon, *dx0;
  float* act[11]; float* dact[2];
  float *dJtr, *dJv, *dtr_j, *gp, *dfp_add;   /* [B][nj][3], [B][n_extra+n_lmk][3], [B][3], [B][81], [B][3 nj] (zeroed once) */
  float *dvp, *dA, *dtr_v, *dX;
  float *g_go, *g_lh, *g_rh, *g_jaw, *g_leye, *g_reye, *g_expr, *g_pe;
  double* loss_acc;               /* [32][32] */
  float* losses;                  /* [16] */
} lemo_prox_desc;
void* lemo_prox_create(const lemo_prox_desc* d);
void lemo_prox_destroy(void* h);
/* forward + backward without the update: losses[] and the g_* / dtr_* buffers (erase applied by the update only) */
int lemo_prox_closure(void* h, void* stream);
/* n iterations (closure + Adam); use_graph as lemo_fit_step */
int lemo_prox_step(void* h, int n, int use_graph, void* stream);
/* Optimiser state of a PROX window (fitting_temp_slide.py:196-204: optimizer.step(closure) x maxiters on the parameters
 * fit_temp_loadprox_slide.py:511-519 collects): the nine optimised tensors in lemo_prox_desc's shapes, Adam's moments as
 * [B][81] blocks in the same order (global_orient 3 | transl 3 | left_hand 12 | right_hand 12 | jaw 3 | leye 3 | reye 3 |
 * expression 10 | pose_embedding 32) and the completed-step count.  Same contract as lemo_fit_load_state / save_state;
 * window k + 1 of a recording is window k's saved parameters on the overlap with a FRESH Adam (data_parser_slide.py:326-331). */
typedef struct lemo_prox_state {
  float *global_orient, *transl, *left_hand_pose, *right_hand_pose, *jaw_pose, *leye_pose, *reye_pose, *expression, *pose_embedding;
  float *adam_m, *adam_v;         /* [B][81] */
  int* step;                      /* [1] */
} lemo_prox_state;
int lemo_prox_load_state(void* h, const lemo_prox_state* st, void* stream);
int lemo_prox_save_state(void* h, const lemo_prox_state* st, void* stream);

/* ---- optional terms of the PROX window engine (csrc/prox_terms_kernels.hip) ------------------------------------------------
 * The terms cfg_files/PROXD_temp_S3.yaml:58-86 switches on top of the S2 / S3 set, as SMPLifyLoss.forward evaluates them: s2m / m2s
 * :637-670, self-penetration :618-635, body-scene contact :743-753, marker acceleration / velocity :756-772.  lemo_prox_set_terms
 * attaches them to a created engine: call it before the first step (a later call drops the captured graphs; the next step captures
 * again).  A term whose weight is 0 or whose pointers are NULL launches nothing; an engine that never sees this call runs exactly the
 * launches of lemo_prox_step above.  In an iteration the terms run behind prox_sparse and in front of the all-vertex backward, add
 * their gradients to lemo_prox_desc.dverts (camera space), fill losses[2, 3, 4, 6, 7, 8] and add those to losses[0] in the order
 * contact, s2m + m2s, self-penetration, acceleration, velocity, so the non-finite latch sees them.
 * Everything below is caller-allocated device memory except contact_vid_host; the engine never allocates or synchronises.  The
 * searches are the entry points further down (lemo_chamfer_forward with LEMO_CHAMFER_SHARED, lemo_vertex_visibility,
 * lemo_chamfer_masked_forward twice, lemo_selfpen_search, lemo_selfpen_loss_forward), inside the capture; they see the iteration's
 * vertices and take no gradient.  The workspaces have the sizes of those entry points' lemo_*_workspace_bytes functions for
 * (B, Nc, M, SHARED, 0), (B, V, F, AUTO, 0), the larger of (B, S, V, 0, 0) and (B, V, S, 0, 0), and (B, V, F, AUTO, 0).
 *   contact   scene_v [M][3] world space, contact_vid [Nc] with a host copy (unique ids in [0, V)): d = squared distance of
 *             R v + t to the nearest scene vertex, s = sqrt(d + 1e-4), contact_loss_weight * mean(s / (s + 1)); the gradient goes
 *             back through R^T to the one dverts row an id owns (no atomics).  Scratch: contact_xyz [B][Nc][3], contact_dist /
 *             contact_idx [B][Nc], contact_ws.
 *   scan      faces [F][3], scan [B][S][3] camera space, scan_point_num [B] (clamped to 0 .. S on the device), body_mask [V] bytes.
 *             vis = lemo_vertex_visibility(verts, min_dist); a frame is live iff it has a scan point and a visible vertex (m2s: and a
 *             vertex with vis & body_mask); per live frame the mean of rho^2 d / (d + rho^2) over the valid scan points against the
 *             visible vertices (s2m) / over the vis & body_mask vertices against the valid scan points (m2s); weight * mean over the
 *             live frames.  Scratch: vis, qmask [B][V] bytes, scan_counts [3][B], s2m_dist / s2m_idx [B][S], m2s_dist / m2s_idx
 *             [B][V], vis_ws, scan_ws.
 *   selfpen   faces, optional segm / parents [F] and ign [P][P] (as lemo_selfpen_search); sum over the frames of coll_loss_weight *
 *             lemo_selfpen_loss_forward.  Scratch: pairs [B][max_pairs][2], pair_count [B], pen_loss [B], pen_ws.
 *   velocity  the markers fit.row81 of the engine: smooth_vel_weight * mean((x[b+1] - x[b])^2) over (B - 1) n81 3 entries and
 *             smooth_acc_weight * mean of the squared second difference over (B - 2) n81 3.
 * The two scattered adjoints (s2m: many scan points share a vertex; self-penetration) are summed in fix_acc [B][V][3][2], fixed point
 * in two 64-bit words per entry (units of 2^-20 and 2^-60, csrc/fixed_acc.hpp) with integer atomics: the sum does not depend on the
 * order of arrival, so graph replay == eager launches bit for bit.  It is zeroed every iteration and added to dverts by the closing
 * kernel.  A contribution that is not finite or not below 2^17 in magnitude is not converted, and neither is a valid scan point that
 * is not finite: either raises fix_flag [1] and the closing kernel makes losses[0] NaN, which latches
 * lemo_prox_desc.nonfinite.  frame_acc [B][8] (double): the per-frame sums behind the loss values.
 * LEMO_ERR_ARG: a NULL handle or struct, a negative or non-finite weight, a live term with a NULL pointer or a workspace smaller than
 * stated, contact ids that repeat or leave [0, V), rho / sigma that are not positive; LEMO_ERR_SHAPE: the limits of the entry points
 * named above for the shapes given.  Nothing is launched and the engine keeps its earlier terms then. */
typedef struct lemo_prox_terms {
  /* contact */
  const float* scene_v; int M;
  const int* contact_vid; const int* contact_vid_host; int Nc;
  float contact_loss_weight;
  float* contact_xyz; float* contact_dist; int* contact_idx;
  void* contact_ws; long long contact_ws_bytes;
  /* the mesh (scan and self-penetration) */
  const int* faces; int F;
  /* scan */
  const float* scan; int S;
  const int* scan_point_num;
  const unsigned char* body_mask;
  float s2m_weight, m2s_weight, rho_s2m, rho_m2s, min_dist;
  unsigned char *vis, *qmask;
  int* scan_counts;
  float* s2m_dist; int* s2m_idx;
  float* m2s_dist; int* m2s_idx;
  void* vis_ws; long long vis_ws_bytes;
  void* scan_ws; long long scan_ws_bytes;
  /* self-penetration */
  const int *segm, *parents; const unsigned char* ign; int P;
  float coll_loss_weight, sigma;
  int penalize_outside, max_pairs;
  int *pairs, *pair_count;
  float* pen_loss;
  void* pen_ws; long long pen_ws_bytes;
  /* marker velocity / acceleration */
  float smooth_acc_weight, smooth_vel_weight;
  /* shared scratch */
  long long* fix_acc;             /* [B][V][3][2]; needed with s2m or self-penetration */
  int* fix_flag;                  /* [1] */
  double* frame_acc;              /* [B][8] */
} lemo_prox_terms;
int lemo_prox_set_terms(void* h, const lemo_prox_terms* t);

/* ---- occlusion masks (csrc/occlusion_kernels.hip): utils/get_occlusion_mask.py:111-147, 170-201 ----
 * Pinhole camera in camera space (y down, z forward): u = fx X / Z + cx, v = fy Y / Z + cy; pixel [y][x] samples the ray through
 * (x + 0.5, y + 0.5).  Depth is the camera-space Z of the nearest hit with znear <= Z <= zfar, 0 where nothing is hit.
 * cull_backface: draw a triangle only if ((v1 - v0) x (v2 - v0)) . v0 < 0 (counter-clockwise as the camera sees it).
 * LEMO_ERR_SHAPE: W or H outside [1, 32768], V / F / T / P < 1, P > 128, T > 65535; LEMO_ERR_ARG: null pointers, intrinsics or
 * depth range that are not positive and finite.  Faces that name a vertex outside [0, V) are skipped. */
typedef struct lemo_occl_cam {
  float fx, fy, cx, cy;
  float znear, zfar;              /* pyrender's defaults: 0.05, 100 */
  int W, H;
  int cull_backface;
} lemo_occl_cam;
/* verts [V][3], faces [F][3] (device); xf: host [12], a rigid transform [R | t] row-major applied to every vertex on load, or NULL;
 * depth [H][W] (device) out.  Order-independent: the same mesh gives the same bits whatever the order of its faces. */
int lemo_depth_raster(const float* verts, int V, const int* faces, int F, const float* xf, const lemo_occl_cam* cam, float* depth,
                      void* stream);
/* verts [T][V][3] (camera space), faces [F][3], points [T][P][3]: the body's depth at the pixel each point projects to (fx = proj_fx,
 * fy = proj_fy, the centre of cam; truncated toward zero like astype(int)), without rendering the body, and the reference's rule
 *   occluded <=> 0 <= x < W and 0 <= y < H and depth_scene[y][x] != 0 and depth_body - depth_scene[y][x] > thresh.
 * depth_scene [H][W] as lemo_depth_raster wrote it for cam; ws [T][P] scratch; mask [T][P] out, 1 = visible; optional outputs (or
 * NULL) depth_body [T][P] (0: the body does not cover the pixel, or the point is outside the image) and pix [T][P][2] = (x, y),
 * INT_MIN where the projection is not finite. */
int lemo_occlusion_query(const float* verts, int T, int V, const int* faces, int F, const float* points, int P, const lemo_occl_cam* cam,
                         float proj_fx, float proj_fy, const float* depth_scene, float thresh, unsigned* ws, float* mask,
                         float* depth_body, int* pix, void* stream);

/* ---- body overlays (csrc/render_kernels.hip): the render_results branch of temp_prox/fit_temp_loadprox_slide.py:622-683 ----
 * The camera, the coverage and the depth are lemo_depth_raster's (same device functions: the depth of a frame is bit for bit what
 * lemo_depth_raster writes for that frame's mesh).  Everything is deterministic: no float atomics, the same bits whatever the order
 * of faces, the number of frames per call or the run.  All memory is the caller's; nothing synchronises.
 * LEMO_ERR_SHAPE: B, V, F, P < 1, B > 65535, F > 2^30, B V > 2^30, W or H outside [1, 32768], radius outside [0, 16], nnz < 0;
 * LEMO_ERR_ARG: null pointers, a camera lemo_depth_raster refuses, shading values outside [0, 1] or not finite, an unknown background
 * kind, a colour above 0xFFFFFF.  Nothing is launched then.
 *
 * lemo_vertex_normals: verts [B][V][3], faces [F][3]; adj_start [V + 1], adj_face [nnz]: for vertex v the faces
 *   adj_face[adj_start[v] .. adj_start[v + 1]) that contain it, in ascending order, each once (the CALLER's to build and to keep
 *   inside [0, F); entries outside it are skipped, as are faces that name a vertex outside [0, V)).  sums [B][V][3] (or NULL): the sum
 *   of (p1 - p0) x (p2 - p0) over those faces in that order; normals [B][V][3] (or NULL): sums / sqrt(sums . sums), (0, 0, 0) where
 *   sums . sums is not > 0.  At least one of the two outputs.
 * lemo_render_ids: verts [B][V][3] in camera space -> keys [B][H][W] (the raster's depth keys, scratch), ids [B][H][W]:
 *   0xFFFFFFFF - f of the lowest-index face f among those whose depth at the pixel is the nearest, 0 where nothing is hit; depth
 *   [B][H][W] (or NULL): camera-space Z, 0 where nothing is hit.
 * lemo_render_resolve: rgb [B][H][W][3] uint8 <- per covered pixel the quantised colour base_k * shade,
 *   shade = min(1, ambient + diffuse |n_z| / |n|) with n the perspective-correct interpolation of the three vertex normals [B][V][3]
 *   (weights e_i / (e0 + e1 + e2) of the face's edge functions at the pixel's ray; 0 instead of |n_z| / |n| where |n| = 0),
 *   q = (int)(255 c + 0.5) clamped to 0 .. 255; per uncovered pixel the background's pixel -- background [B][H][W][3], or [H][W][3]
 *   with bg_shared, of uint8 (LEMO_RENDER_BG_U8) or of float32 in [0, 1] quantised by the same rule (LEMO_RENDER_BG_F32; a NaN gives
 *   0) -- or (0, 0, 0) with LEMO_RENDER_BG_NONE.  Optional (or NULL): face_ids [B][H][W] int32, -1 where nothing is hit; shade
 *   [B][H][W], 0 where nothing is hit.  ids as lemo_render_ids wrote them for the same verts, faces and cam.
 * lemo_render_points: points [B][P][2] pixel coordinates (u, v); x = trunc(u), y = trunc(v); every pixel (x + i, y + j) with
 *   i^2 + j^2 <= radius^2 inside the image gets color (0xRRGGBB).  Points that are not finite (or do not fit an int) are skipped. */
typedef struct lemo_render_shade {
  float base[3];                  /* base colour, each in [0, 1] */
  float ambient, diffuse;         /* each in [0, 1] */
} lemo_render_shade;
#define LEMO_RENDER_BG_NONE 0
#define LEMO_RENDER_BG_U8 1
#define LEMO_RENDER_BG_F32 2
int lemo_vertex_normals(const float* verts, int B, int V, const int* faces, int F, const int* adj_start, const int* adj_face, int nnz,
                        float* normals, float* sums, void* stream);
int lemo_render_ids(const float* verts, int B, int V, const int* faces, int F, const lemo_occl_cam* cam, unsigned* keys, unsigned* ids,
                    float* depth, void* stream);
int lemo_render_resolve(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam,
                        const unsigned* ids, const lemo_render_shade* shade_par, const void* background, int bg_kind, int bg_shared,
                        unsigned char* rgb, int* face_ids, float* shade, void* stream);
int lemo_render_points(const float* points, int B, int P, int radius, int W, int H, unsigned color, unsigned char* rgb, void* stream);

/* ---- 3-D views of fitted bodies (csrc/view_kernels.hip): temp_prox/renderer.py '3d' mode, temp_prox/viz/viz_fitting.py,
 * vis_opt_amass.py -- the body inside the coloured scene mesh, markers as spheres.  The rules are written out in
 * lemo_amd/scene_view.py.  Deterministic, no atomics of their own; all memory is the caller's; nothing synchronises.
 * LEMO_ERR_SHAPE: n, B, V, F < 1, n > 2^30, B > 65535, F > 2^30, B V > 2^30, P outside [0, 256], W or H outside [1, 32768];
 * LEMO_ERR_ARG: null pointers, a camera lemo_depth_raster refuses, a transform that is not finite, shading values outside [0, 1], a
 * colour above 0xFFFFFF, a scene key without scene rgb or the reverse.  Nothing is launched then.
 *
 * lemo_view_transform: points [n][3] -> out [n][3], each through xf (host [12], [R | t] row-major) as lemo_depth_raster applies its
 *   xf on load: ((m0 x + m1 y) + m2 z) + m3 per row.
 * lemo_view_scene_resolve: the static layer of one view.  verts [V][3] in camera space, normals [V][3] (may be NULL when lit == 0),
 *   ids [H][W] as lemo_render_ids wrote them for B = 1, colors [V][3] uint8 -> rgb [H][W][3]: per covered pixel
 *   q(((b0 C0 + b1 C1) + b2 C2) shade), C = uint8 / 255, b_i the weights lemo_render_resolve interpolates normals with,
 *   shade = lemo_render_resolve's (1 when lit == 0); (0, 0, 0) where nothing is hit.
 * lemo_view_compose: B frames.  verts, normals [B][V][3] (camera space), keys, ids [B][H][W] as lemo_render_ids wrote them;
 *   scene_key [H][W] (the keys lemo_render_ids left for the scene) with scene_rgb [H][W][3], or both NULL; spheres [B][P][3] in world
 *   coordinates (or P = 0), sent through view (host [12], or NULL for the identity), radius [P], sphere_rgb [P][3] (rgb_shared) or
 *   [B][P][3].  A sphere is hit analytically: A = d . d, q = c x d, disc = A r^2 - q . q >= 0, Z = (d . c - sqrt(disc)) / A inside
 *   [znear, zfar]; spheres with a centre or radius that is not finite, r <= 0 or c_z - r < znear are not drawn.  Per pixel the
 *   nearest of the three layers wins (equal depth: body, spheres by lowest index, scene); rgb [B][H][W][3]: the body shaded as
 *   lemo_render_resolve does, a sphere by its own normal and colour, the scene's rgb, or bg (0xRRGGBB); optional (or NULL) depth
 *   [B][H][W] (0: nothing) and owner [B][H][W] (-1 nothing, 0 scene, 1 body, 2 + s sphere s). */
int lemo_view_transform(const float* points, long long n, const float* xf, float* out, void* stream);
int lemo_view_scene_resolve(const float* verts, const float* normals, int V, const int* faces, int F, const lemo_occl_cam* cam,
                            const unsigned* ids, const unsigned char* colors, float ambient, float diffuse, int lit, unsigned char* rgb,
                            void* stream);
int lemo_view_compose(const float* verts, const float* normals, int B, int V, const int* faces, int F, const lemo_occl_cam* cam,
                      const unsigned* keys, const unsigned* ids, const lemo_render_shade* shade_par, const unsigned* scene_key,
                      const unsigned char* scene_rgb, const float* spheres, int P, const float* radius, const unsigned char* sphere_rgb,
                      int rgb_shared, const float* view, unsigned bg, unsigned char* rgb, float* depth, int* owner, void* stream);

/* ---- Chamfer nearest neighbours (csrc/chamfer_kernels.hip): the `chamfer` extension of temp_prox/dist_chamfer.py:27,43 and the
 * scene-contact term of fitting_temp_slide.py:743-753 ----
 * xyz1 [B][N][3], xyz2 [B][M][3] (or [1][M][3] with LEMO_CHAMFER_SHARED: one target set for every batch entry, never copied); fp32,
 * contiguous, finite.  dist1 [B][N] = the SQUARED distance (dx dx + dy dy) + dz dz of the differences to a nearest point of xyz2,
 * idx1 [B][N] its index; ties go to the lowest index.  With LEMO_CHAMFER_REVERSE also dist2 / idx2 [B][M] (xyz2 against xyz1);
 * otherwise they are not touched and may be NULL.  SHARED | REVERSE is refused (LEMO_ERR_ARG): that direction is not defined.
 * split: 0 = automatic, k > 0 = cut the target range into (at most) k pieces; results do not depend on it, bit for bit.
 * ws: lemo_chamfer_workspace_bytes(same B, N, M, flags, split) bytes of device scratch (0 bytes: may be NULL).
 * LEMO_ERR_SHAPE: B, N or M < 1, B > 65535, B N or B M > 2^30; LEMO_ERR_ARG: null pointers, unknown flags, split < 0, a
 * workspace that is too small.  Nothing is allocated and nothing synchronises. */
#define LEMO_CHAMFER_SHARED 1
#define LEMO_CHAMFER_REVERSE 2
long long lemo_chamfer_workspace_bytes(int B, int N, int M, int flags, int split);      /* -1 for arguments the forward refuses */
int lemo_chamfer_forward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, int split, float* dist1, int* idx1,
                         float* dist2, int* idx2, void* ws, long long ws_bytes, void* stream);
/* grad1[b][i] = 2 g1[b][i] (x1[b][i] - x2[b][idx1[b][i]]) + sum over {j : idx2[b][j] == i} of 2 g2[b][j] (x1[b][i] - x2[b][j]) and the mirror
 * image for grad2 ([1][M][3], summed over the batch too, with LEMO_CHAMFER_SHARED).  g2 / idx2 are read only with LEMO_CHAMFER_REVERSE.
 * grad1 / grad2 need no initialisation; a NULL one is neither computed nor written.  The scattered sums are fp32 atomic adds. */
int lemo_chamfer_backward(const float* xyz1, const float* xyz2, int B, int N, int M, int flags, const float* g1, const int* idx1,
                          const float* g2, const int* idx2, float* grad1, float* grad2, void* stream);
/* out4 (host): queries per workgroup, targets per LDS chunk, the fewest targets an automatic split holds, and the number of
 * workgroups at which the automatic split stops cutting the target range */
void lemo_chamfer_sizes(int* out4);
/* The one-sided search where every batch entry has its own valid points (the s2m / m2s terms, fitting_temp_slide.py:657-667).
 * Query i of entry b is valid iff (n1 == NULL or i < n1[b]) and (q_mask == NULL or q_mask[b][i] != 0); target j likewise with n2 /
 * t_mask.  n1, n2: int32 [B]; q_mask [B][N], t_mask [B][M]: bytes; all on the device, any of them NULL.  dist1 / idx1 [B][N]: the
 * nearest VALID target (index into the original array, lowest index on ties); dist 0 and idx -1 for an invalid query and for every
 * query of an entry without a valid target -- lemo_chamfer_backward(flags = 0) gives such a query no gradient.  split and ws as for
 * lemo_chamfer_forward with lemo_chamfer_workspace_bytes(B, N, M, 0, split); results do not depend on split, bit for bit, and equal
 * lemo_chamfer_forward's when everything is valid.  Same error codes. */
int lemo_chamfer_masked_forward(const float* xyz1, const float* xyz2, int B, int N, int M, const int* n1, const unsigned char* q_mask,
                                const int* n2, const unsigned char* t_mask, int split, float* dist1, int* idx1, void* ws, long long ws_bytes,
                                void* stream);

/* ---- body-vertex visibility (csrc/visibility_kernels.hip): psbody.mesh.visibility.visibility_compute(v, f, cams) with min_dist, no
 * normals or sensors, for B frames at once (fitting_temp_slide.py:642-652) ----
 * verts [B][V][3], faces [F][3] (shared by the frames), cam [B][3] or NULL (the origin); fp32 / int32 on the device.
 * vis [B][V] bytes out, 1 = visible: the segment from p + min_dist (c - p) / |c - p| to the camera c meets no triangle of the frame
 * (either side, triangles at the vertex included; degenerate triangles never hit; |c - p| <= min_dist is visible).
 * mode: LEMO_VIS_BRUTE tests every pair; LEMO_VIS_BINNED bins the projected vertices of every frame that lies in front of the camera
 * into a grid x grid raster (grid 0 = 64, else 2 .. 64) and lets a frame that does not take the brute-force path; LEMO_VIS_AUTO picks
 * the faster of the two at the PROX shape.  The result does not depend on mode or grid, bit for bit.
 * nbig [B] (or NULL): the number of triangles of each frame that took the one-workgroup-per-triangle pass (0 for brute force).
 * ws: lemo_vertex_visibility_workspace_bytes(same B, V, F, mode, grid) bytes of device scratch (0 bytes: may be NULL).
 * LEMO_ERR_SHAPE: B, V or F < 1, B > 65535, F > 2^30, B V > 2^30; LEMO_ERR_ARG: null pointers, an unknown mode or grid, a min_dist
 * that is negative or not finite, a workspace that is too small.  Faces that name a vertex outside [0, V) never hit. */
#define LEMO_VIS_AUTO 0
#define LEMO_VIS_BRUTE 1
#define LEMO_VIS_BINNED 2
long long lemo_vertex_visibility_workspace_bytes(int B, int V, int F, int mode, int grid);      /* -1 for arguments the launch refuses */
int lemo_vertex_visibility(const float* verts, int B, int V, const int* faces, int F, const float* cam, float min_dist, int mode, int grid,
                           unsigned char* vis, int* nbig, void* ws, long long ws_bytes, void* stream);

/* ---- depth frames to body scans (csrc/depth_scan_kernels.hip): Projection.create_scan (temp_prox/projection_utils.py:35-90) and the
 * truncate / pad / mean of temp_prox/data_parser_slide.py:283-323, for B frames of H x W depth pixels at once ----
 * The calibration: rays [H][W][2] (device, fp32): the undistorted normalised IR coordinate of every depth pixel (built once per
 * calibration on the host); everything else is host data, row-major: view_d = [R_d | t_d] (3 x 4) of the IR camera; Rc (3 x 3, from
 * the colour camera's Rodrigues vector), Tc, fx / fy / cx / cy, k = (k1, k2, p1, p2, k3) of the colour camera; view_c (3 x 4) its view
 * matrix; cW x cH the colour image. */
typedef struct lemo_depth_calib {
  const float* rays;
  float view_d[12];
  float Rc[9], Tc[3];
  float fx, fy, cx, cy;
  float k[5];
  float view_c[12];
  int cW, cH;
} lemo_depth_calib;
/* depth [B][H][W]: float32 metres (raw = 0) or uint16 with d = raw / 8 * depth_scale (raw = 1); flip = 1 reads the frame mirrored
 * left-right.  mask: bytes, [B][cH][cW] looked up at the rounded colour pixel (mask_on_color = 1), or [B][H][W] with the depth taken as
 * 0 where it is non-zero (mask_on_color = 0; the caller's depth is not modified).  A pixel is valid iff its depth is finite, the z of
 * its point exceeds TH and, with mask_on_color, its colour pixel lies inside the image and the mask is 0 there.  coord_color = 1 gives
 * points in the colour camera's frame (view_c . (p, 1)), 0 the unprojected p.
 * Out: scan [B][S][3]: the first S valid points of each frame in row-major pixel order, zeros behind them (no initialisation
 * needed); n_valid [B]: the valid pixels; scan_point_num [B] = min(n_valid, S); init_trans [B][3]: the mean of ALL valid points (NaN
 * without any); optionally (both or neither) points [B][H][W][3] and valid [B][H][W]: every pixel's point and flag -- the scan holds
 * exactly those bits.  Deterministic.  ws: lemo_depth_scan_ws_bytes(B, H, W) bytes of device scratch, 8-byte aligned.
 * LEMO_ERR_SHAPE: B, H, W or S < 1, B > 1024, H W > 2^22, S > 2^20, cW or cH outside [1, 32768]; LEMO_ERR_ARG: null pointers, a flag
 * that is not 0 / 1, depth_scale or TH not finite, a workspace that is too small.  Nothing is launched then. */
long long lemo_depth_scan_ws_bytes(int B, int H, int W);      /* -1 for shapes the launch refuses */
int lemo_depth_scan(const void* depth, int raw, int flip, float depth_scale, const unsigned char* mask, int mask_on_color, int coord_color,
                    float TH, const lemo_depth_calib* cal, int B, int H, int W, int S, float* scan, int* scan_point_num, int* n_valid,
                    float* init_trans, float* points, unsigned char* valid, void* ws, long long ws_bytes, void* stream);
/* points [B][H][W][3] = unproject_depth_image of every frame (projection_utils.py:35-48); the colour camera's fields are not read */
int lemo_depth_unproject(const void* depth, int raw, int flip, float depth_scale, const lemo_depth_calib* cal, int B, int H, int W,
                         float* points, void* stream);

/* ---- self-penetration (csrc/selfpen_kernels.hip): mesh_intersection's BVH search + FilterFaces + DistanceFieldPenetrationLoss
 * (fitting_temp_slide.py:618-635) for B frames at once; the behaviour is the one written in that file's header, not a run of the
 * package ----
 * verts [B][V][3] fp32, faces [F][3] int32 (shared by the frames); optional segm [F], parents [F] (int32) and ign [P][P] bytes
 * (P <= 64; parents and ign need segm).  Triangles i < j of a frame collide iff they share no vertex index, their boxes overlap, an
 * edge of one meets the other (Moeller-Trumbore, inclusive, either side, a zero determinant never hits) and the segmentation does
 * not exclude them; a face with a vertex outside [0, V) or a coordinate that is not finite never collides.
 * pairs [B][C][2] out: the colliding pairs in lexicographic order, -1 behind the last, the first C on overflow; count [B] out: the
 * true number (saturates at 2^31 - 1).  Deterministic, no host synchronisation, no allocation.  mode: LEMO_SELFPEN_BRUTE tests
 * every pair behind a box reject, LEMO_SELFPEN_GRID bins the faces of every frame into a grid^3 lattice (grid 0 = 16, else 2 .. 16),
 * LEMO_SELFPEN_AUTO picks the faster at the PROX shape; the result does not depend on mode or grid, bit for bit.
 * ws: lemo_selfpen_search_workspace_bytes(same B, V, F, mode, grid) bytes of device scratch.
 * LEMO_ERR_SHAPE: B, V, F or C < 1, B > 65535, F > 2^24, B V or B F > 2^30, B C > 2^28; LEMO_ERR_ARG: null pointers, an unknown mode
 * or grid, P outside 0 .. 64 or inconsistent with ign, a workspace that is too small.  Nothing is launched then. */
#define LEMO_SELFPEN_AUTO 0
#define LEMO_SELFPEN_BRUTE 1
#define LEMO_SELFPEN_GRID 2
long long lemo_selfpen_search_workspace_bytes(int B, int V, int F, int mode, int grid);         /* -1 for arguments the launch refuses */
int lemo_selfpen_search(const float* verts, int B, int V, const int* faces, int F, const int* segm, const int* parents, const unsigned char* ign,
                        int P, int mode, int grid, int* pairs, int C, int* count, void* ws, long long ws_bytes, void* stream);
/* loss [B] out: the cone distance field of the receiving triangle at the intruding triangle's corners, squared, both ways, summed
 * over the first min(count[b], C) pairs of each frame (count NULL: all C; an entry that names no face is skipped).  sigma > 0.
 * Deterministic.  A zero-area triangle contributes nothing. */
int lemo_selfpen_loss_forward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                              int penalize_outside, float* loss, void* stream);
/* gverts [B][V][3] out (zeroed here) = sum_b gloss[b] dL[b] / dverts: through the points and through the normal, circumcentre and
 * circumradius of the receiving triangles; fp32 atomic adds. */
int lemo_selfpen_loss_backward(const float* verts, int B, int V, const int* faces, int F, const int* pairs, int C, const int* count, float sigma,
                               int penalize_outside, const float* gloss, float* gverts, void* stream);

/* ---- scene signed-distance volume (csrc/scene_sdf_kernels.hip): a triangle mesh -> the sdf / grid_min / grid_max that lemo_sdf_sample, the
 * PROX engine and ProxTemporalFitter take.  The definition is this project's (that file's header states it in full); the program that
 * made PROX's own <scene>_sdf.npy was never published ----
 * verts [V][3] fp32, faces [F][3] int32.  Tables, built once per mesh by the caller (float64, rounded to fp32): face_n [F][3] unit face
 * normals, ALL ZERO for a triangle to be ignored (zero area); edge_n [F][3][3]: for edge e of face f (0: v0 v1, 1: v1 v2, 2: v2 v0) the
 * sum of the unit normals of the faces sharing that undirected edge; vert_n [V][3]: the incident faces' unit normals weighted by their
 * corner angles.  A triangle with a vertex index outside [0, V) or a coordinate that is not finite is ignored as well.
 * gmin, gmax: host float[3], finite, gmin < gmax.  Out: sdf [D][H][W] (x, y, z) at the voxel centres gmin + (i + 0.5) (gmax - gmin) / dim:
 * the exact distance to the nearest point of the mesh, negative where (p - c) . n < 0 for the closest point c and the pseudonormal n
 * of the feature it lies on; +inf everywhere without a valid triangle.  nearest (or NULL) [D][H][W]: the winning face (smallest squared
 * distance, then lowest index; -1 without one).  mode: LEMO_SCENE_SDF_BRUTE streams every triangle past every voxel,
 * LEMO_SCENE_SDF_GRID searches a grid^3 cell grid outward (grid 0 = max(D, H, W) / 8 clamped to 2 .. 32, else 2 .. 32),
 * LEMO_SCENE_SDF_AUTO is GRID except for tiny meshes; the output does not depend on mode or grid, bit for bit, and repeated runs are
 * bit-identical.  ws: lemo_scene_sdf_ws_bytes(F, D, H, W, mode, grid) bytes of device scratch (0 for brute force: ws may be NULL).
 * No allocation, no host synchronisation, capturable in a graph.
 * LEMO_ERR_SHAPE: F, V, D, H or W < 1, a side > 1024, D H W > 2^28, F > 2^22, V > 2^24; LEMO_ERR_ARG: null pointers, an unknown mode or
 * grid, bounds that are not finite or empty, a workspace that is too small.  Nothing is launched then. */
#define LEMO_SCENE_SDF_AUTO 0
#define LEMO_SCENE_SDF_BRUTE 1
#define LEMO_SCENE_SDF_GRID 2
long long lemo_scene_sdf_ws_bytes(int F, int D, int H, int W, int mode, int grid);               /* -1 for arguments the launch refuses */
int lemo_scene_sdf_build(const float* verts, int V, const int* faces, int F, const float* face_n, const float* edge_n, const float* vert_n,
                         const float* gmin, const float* gmax, int D, int H, int W, int mode, int grid, float* sdf, int* nearest, void* ws,
                         long long ws_bytes, void* stream);

/* ---- L-BFGS with a strong-Wolfe line search (csrc/lbfgs_kernels.hip, csrc/lbfgs_host.hpp) -----------------------------------
 * The optimiser `optim_type: 'lbfgsls'` of the PROX configs selects (temp_prox/optimizers/lbfgs_ls.py): one step = up to max_iter
 * quasi-Newton iterations, each a two-loop recursion over a ring of `history` (y, s) pairs and a bracket-then-zoom search on cubic
 * interpolants.  A generic object over flat fp32 vectors of n elements in CALLER-OWNED device memory:
 *   ws = lemo_lbfgs_ws_bytes(n, history) bytes (-1 for n outside 1 .. 32768 or history outside 1 .. 128), 8-byte aligned, alive as
 *   long as the object.  lemo_lbfgs_create returns NULL for a refused n / history, a NULL or short ws, max_iter < 1, or lr, c1, c2,
 *   tolerance_grad, tolerance_change that are not positive and finite.  max_eval <= 0 means max_iter * 5 / 4, max_ls <= 0 means 25.
 * One `optimizer.step(closure)`, with the closure evaluated by the caller:
 *   lemo_lbfgs_begin(h, x, g, f_dev, stream)   x [n], its gradient g [n], its loss f_dev [1] (fp32, device): starts a step
 *   lemo_lbfgs_ask(h, x_trial, stream)         LEMO_LBFGS_EVAL: evaluate x_trial [n] and call lemo_lbfgs_tell;
 *                                              LEMO_LBFGS_DONE: x_trial is the accepted point, the step is over;
 *                                              a NEGATIVE value: minus the error code
 *   lemo_lbfgs_tell(h, g, f_dev, stream)       gradient and loss of the last x_trial
 * The memory, the iteration count and the last (d, t) persist from step to step, as the reference's `state` does.
 * SYNCHRONISATION: lemo_lbfgs_ask and lemo_lbfgs_tell wait for `stream` (and only for it) -- the `float(closure())` of the
 * reference: a decision needs the loss and g.d on the host.  They are read back through a pinned word.  These two (and
 * lemo_prox_lbfgs_step, which calls them) are the only entry points of the library that synchronise.
 * Arithmetic: vectors fp32; every dot product in double in the fixed order of one workgroup (no atomics: two runs agree bit for
 * bit); the scalars of the search in double on f (the caller's fp32, widened) and the device's double g.d.
 * NON-FINITE LOSS (a rule of ours; the reference is undefined there): a non-finite f at lemo_lbfgs_begin moves nothing, ends the step
 * (stop reason 8) and latches: every later step ends at once.  A non-finite trial f inside a search counts as "sufficient decrease
 * failed".
 * lemo_lbfgs_trace: rows of 8 doubles, one per evaluation since create, into out[cap][8]; returns the number of rows recorded (at
 * most 4096 are kept), or a negative error: iteration (1-based, over the object's life), phase (0 = the step's opening closure, 1 =
 * bracketing trial, 2 = zoom trial), t, f, g.d, max|g|, accepted (1: the point a search ended at, or the step's start), stop reason of
 * the step (1 max|g| <= tolerance_grad at the start, 2 g.d > -tolerance_change, 3 max_iter, 4 max_eval, 5 max|g| <= tolerance_grad,
 * 6 max|t d| <= tolerance_change, 7 |f - f_prev| < tolerance_change, 8 non-finite).
 * lemo_lbfgs_set_log (diagnostics): xlog / dlog [cap_rows][n] receive the point and the direction of every traced evaluation (device
 * copies on `stream`; dlog may be NULL; cap_rows 0 switches it off).
 * LEMO_ERR_ARG: null pointers; LEMO_ERR_STATE: calls out of order. */
#define LEMO_LBFGS_EVAL 1
#define LEMO_LBFGS_DONE 2
typedef struct lemo_lbfgs_opts {
  double lr, c1, c2, tolerance_grad, tolerance_change;      /* the reference: lr 1, 1e-4, 0.9, 1e-5, 1e-9 */
  int max_iter, max_eval, max_ls, history;                  /* the reference: 20 (PROX: 30), max_iter * 5 / 4, 25, 100 */
} lemo_lbfgs_opts;
long long lemo_lbfgs_ws_bytes(int n, int history);
void* lemo_lbfgs_create(int n, const lemo_lbfgs_opts* opts, void* ws, long long ws_bytes);
void lemo_lbfgs_destroy(void* h);
int lemo_lbfgs_begin(void* h, const float* x, const float* g, const float* f_dev, void* stream);
int lemo_lbfgs_ask(void* h, float* x_trial, void* stream);
int lemo_lbfgs_tell(void* h, const float* g, const float* f_dev, void* stream);
int lemo_lbfgs_trace(void* h, double* out, int cap);
int lemo_lbfgs_set_log(void* h, float* xlog, float* dlog, int cap_rows);
/* the direction kernel on caller buffers (one launch, one workgroup; asynchronous): memory update y = g - g_prev, s = t d, pushed into
 * the ring Y / Sv [history][n], ro [history] when y.s > 1e-10 (ring [2] = head, count; hdiag [1] = y.s / y.y; all on the device, the
 * branch is taken there), two-loop recursion, g_prev <- g, d out, and rec [8] doubles: g.d, sum|g|, max|g|, max|d|, y.s, y.y,
 * H_diag, ring count.  first != 0: d = -g and the ring is emptied.  LEMO_ERR_SHAPE: n outside 1 .. 32768, history outside 1 .. 128;
 * LEMO_ERR_ARG: null pointers, a non-finite t. */
int lemo_lbfgs_direction(int n, int history, int first, double t, const float* g, float* g_prev, float* d, float* Y, float* Sv, double* ro,
                         double* hdiag, int* ring, double* rec, void* stream);
/* n x `optimizer.step(closure)` of a PROX window engine under L-BFGS (`lbfgs` created for 81 B elements: frame-major [B][81] in the
 * engine's parameter order).  One evaluation is x = x0 + t d, its scatter into the nine parameter tensors, the engine's closure (with
 * the optional terms when attached), the flat gradient (priors included, the first int(0.15 B) frames zeroed unless first_batch_flag)
 * -- captured once and replayed with use_graph -- then the probe and one read-back.  SYNCHRONOUS (see above).  After a step whose
 * opening loss is not finite, nonfinite[0] latches the 1-based index of that step and the remaining steps do nothing.
 * LEMO_ERR_ARG: null handles, n < 0; LEMO_ERR_SHAPE: `lbfgs` created for another size. */
int lemo_prox_lbfgs_step(void* prox, void* lbfgs, int n, int use_graph, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
