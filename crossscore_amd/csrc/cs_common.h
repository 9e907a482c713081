// Shared device/host helpers for the CrossScore gfx950 kernels.  gfx950 (CDNA4) only: wave64, MFMA with IEEE half (fp16)
// operands and fp32 accumulation (v_mfma_f32_*_f16 runs at the bf16 rate; 11 significant bits instead of 8),
// 160 KiB LDS per CU.  No portability layer on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t h16_t;  // raw fp16 (IEEE binary16) bits in memory

typedef _Float16 h16x8_t __attribute__((ext_vector_type(8)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define CS_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define CS_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// fp32 -> fp16 round-to-nearest-even (v_cvt_f16_f32 / v_cvt_pk_f16_f32 on gfx950; NaN stays NaN, |x| > 65504 becomes inf: the
// range every 16-bit activation of this path has to stay in is stated in DESIGN.md 2 and tested with scaled-up weights).
__device__ __forceinline__ h16_t f2h(float x) {
  _Float16 b = (_Float16)x;
  return __builtin_bit_cast(h16_t, b);
}
__device__ __forceinline__ float h2f(h16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
// two values in one v_cvt_pk_f16_f32 (same round-to-nearest-even as f2h)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_h16x2(float lo, float hi) {
  const h16x2_t v = __builtin_convertvector(f32x2_t{lo, hi}, h16x2_t);
  return __builtin_bit_cast(uint32_t, v);
}

// fp32 score -> the 16-bit code the gray writer stores (metric_map_write, utils/io/images.py:49-63): m*65535 for the [0,1] intrinsic range,
// (m+1)*32767 for [-1,1], truncated toward zero like astype(int32) (the conversion saturates, NaN gives 0), clipped to [0, 65535].  The one
// definition behind score_gray16_kernel (preprocess.hip) and the pooling kernels (scorepool.hip).
__device__ __forceinline__ uint32_t cs_score_code(float m, int signed_range) {
  const float v = signed_range ? (m + 1.0f) * 32767.0f : m * 65535.0f;
  const int q = (int)v;
  return (uint32_t)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
}

// ---- operand type of the MFMA kernels: IEEE half (default) or bfloat16 (cs_config.operand_dtype).  Both are 16 bits in memory (h16_t holds
//      the raw bits either way), both MFMA forms take the same cycles; half carries 11 significant bits and is finite to 65504, bfloat16
//      8 bits with fp32's range.  Kernels with MFMAs take the choice as a template parameter, the memory-bound ones as an argument. ----
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950; a NaN stays a NaN)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ h16_t f2bf(float x) { return __builtin_bit_cast(h16_t, (__bf16)x); }
__device__ __forceinline__ float bf2f(h16_t b) { return __uint_as_float((uint32_t)b << 16); }
template <bool BF> __device__ __forceinline__ uint32_t pack_o16x2(float lo, float hi) {
  if constexpr (BF) return pack_bf16x2(lo, hi);
  else return pack_h16x2(lo, hi);
}
template <bool BF> __device__ __forceinline__ h16_t f2o(float x) {
  if constexpr (BF) return f2bf(x);
  else return f2h(x);
}
template <bool BF> __device__ __forceinline__ float o2f(h16_t b) {
  if constexpr (BF) return bf2f(b);
  else return h2f(b);
}
// run-time forms for the memory-bound kernels (a wave-uniform select)
__device__ __forceinline__ uint32_t pack_o16x2(float lo, float hi, int bf) { return bf ? pack_bf16x2(lo, hi) : pack_h16x2(lo, hi); }
__device__ __forceinline__ h16_t f2o(float x, int bf) { return bf ? f2bf(x) : f2h(x); }
__device__ __forceinline__ float o2f(h16_t b, int bf) { return bf ? bf2f(b) : h2f(b); }
// fragments are carried as h16x8_t (raw bits) in both modes
template <bool BF> __device__ __forceinline__ f32x4_t mfma_16x16x32(const h16x8_t& a, const h16x8_t& b, const f32x4_t& c) {
  if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
template <bool BF> __device__ __forceinline__ f32x16_t mfma_32x32x16(const h16x8_t& a, const h16x8_t& b, const f32x16_t& c) {
  if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// wave64 butterfly reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// GELU(x) = x * Phi(x) with the exact (erf) Phi of HF ACT2FN["gelu"] (HF modeling_dinov2.py:293-297) approximated by
// Phi(x) ~ 0.5 + x * P(x^2), x clamped to +-4.2; P is a degree-7 minimax fit of the GELU error:
// max |GELU_fit - GELU_erf| = 6.7e-5 (2.1e-4 as evaluated in fp32 Horner form, near |x| = 4 where y ~ x; an fp16 half-ulp is
// 4.9e-4 at |y| = 1 and 2e-3 at 4).  The factor in front of Phi is clamped from below as well: y = max(x, -4.2) * Phi_fit(clamp(x, +-4.2)).
// Phi_fit(-4.2) is 3.0e-5, not 0, so below -4.2 the result is the constant -4.2 * 3.0e-5 = -1.26e-4 (the true GELU is -0 there) and the
// 2.1e-4 holds for every finite x <= 4.2.  Above 4.2 y = x * Phi_fit(4.2) = x (1 - 3.0e-5): a relative error, below the 16-bit store's
// half ulp.  (tests/test_hip_activations.py and tests/test_gelu_pk16.py evaluate it on every finite 16-bit input.)
// Non-finite pre-activations: +inf gives FLT_MAX (1 - 3.0e-5), which the store rounds to inf in both 16-bit types; -inf gives the tail;
// a NaN comes out as the tail -1.26e-4, NOT as NaN (v_med3_f32 with a NaN operand returns the smallest of the three): an fc1 that has
// diverged does not show as NaN behind this epilogue.
// Plain VALU ops only (the lower clamp of the factor is a second v_med3_f32 per value), no
// transcendentals: the fc1 epilogue was spending more issue slots on erf (v_exp + v_rcp) than its K loop on MFMAs
// (PMC: SQ_ACTIVE_INST_VALU 51 % vs MFMA pipe busy 26 % with the Abramowitz-Stegun erf).
// Four values per call as two packed-fp32 Horner chains (v_pk_fma_f32) issued alternately from one asm block: a lone chain pays
// a dependent-issue bubble on every packed fma, and the compiler's scheduler serialises the chains again whatever the source
// order.  The fitted Phi stays inside [-1.2e-6, 1 + 1.2e-6] on the clamped range, so it is not clamped again.
__device__ __forceinline__ unsigned long long gelu_c(float c) { return (unsigned long long)__float_as_uint(c); }
__device__ __forceinline__ void gelu_erf4(float (&v)[4]) {
  // max(x, -4.2) as a second v_med3_f32, the median of x, -4.2 and FLT_MAX (x itself for every finite x >= -4.2): fmaxf (and a median
  // with +inf, which hipcc folds into it) costs two instructions per value here -- x comes straight out of an MFMA accumulator and gets a
  // canonicalising v_max_f32 x, x in front
  const float kMax = 3.402823466e+38f;
  const f32x2_t xa = {__builtin_amdgcn_fmed3f(v[0], -4.2f, kMax), __builtin_amdgcn_fmed3f(v[1], -4.2f, kMax)};
  const f32x2_t xb = {__builtin_amdgcn_fmed3f(v[2], -4.2f, kMax), __builtin_amdgcn_fmed3f(v[3], -4.2f, kMax)};
  const f32x2_t ca = {__builtin_amdgcn_fmed3f(v[0], -4.2f, 4.2f), __builtin_amdgcn_fmed3f(v[1], -4.2f, 4.2f)};
  const f32x2_t cb = {__builtin_amdgcn_fmed3f(v[2], -4.2f, 4.2f), __builtin_amdgcn_fmed3f(v[3], -4.2f, 4.2f)};
  const f32x2_t ta = ca * ca, tb = cb * cb;
  const f32x2_t c1 = {8.3297297734e-08f, 8.3297297734e-08f};
  f32x2_t qa, qb;
  // q = c0*t + c1, then q = q*t + c_k: the scalar operand is a register pair whose low half is broadcast (op_sel_hi 0)
  // (leading / trailing s_nop: the packed-fma result hazard against the compiler's own neighbouring instructions)
  asm("s_nop 0\n\t"
      "v_pk_fma_f32 %0, %2, %4, %5 op_sel_hi:[1,0,0]\n\t"
      "v_pk_fma_f32 %1, %3, %4, %5 op_sel_hi:[1,0,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %6 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %6 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %7 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %7 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %8 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %8 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %9 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %9 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %10 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %10 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %0, %0, %2, %11 op_sel_hi:[1,1,0]\n\t"
      "v_pk_fma_f32 %1, %1, %3, %11 op_sel_hi:[1,1,0]\n\t"
      "s_nop 0"
      : "=&v"(qa), "=&v"(qb)
      : "v"(ta), "v"(tb), "s"(gelu_c(-9.6129670387e-10f)), "v"(c1), "s"(gelu_c(-3.1398569575e-06f)), "s"(gelu_c(6.8266010957e-05f)),
        "s"(gelu_c(-9.6075936689e-04f)), "s"(gelu_c(9.3374518106e-03f)), "s"(gelu_c(-6.5599355124e-02f)), "s"(gelu_c(3.9850871469e-01f)));
  const f32x2_t ya = xa * __builtin_elementwise_fma(ca, qa, f32x2_t{0.5f, 0.5f});
  const f32x2_t yb = xb * __builtin_elementwise_fma(cb, qb, f32x2_t{0.5f, 0.5f});
  v[0] = ya[0]; v[1] = ya[1]; v[2] = yb[0]; v[3] = yb[1];
}

// ---- kernel parameter blocks (plain structs; launchers live in the matching .hip files) -------------
enum CsEpilogue {
  CS_EPI_BIAS_F16 = 0,        // out_f16[m][n] = acc + bias[n]
  CS_EPI_BIAS_GELU_F16 = 1,   // erf-GELU, degree-7 minimax fit of Phi (gelu_erf4 above: max abs error 2.1e-4 in fp32 for x <= 4.2, -1.26e-4 below -4.2)
  CS_EPI_BIAS_RELU_F16 = 2,
  CS_EPI_BIAS_LEAKY_F16 = 3,  // slope 0.01
  CS_EPI_RESID_F32 = 4,        // out_f32[m][n] = (resid? resid[m][n]:0) + (scale? scale[n]:1)*(acc+bias[n])
  CS_EPI_PATCH_F32 = 5,        // out_f32[(m + m/Np + 1)][n] = acc + bias[n] + pos[(m%Np+1)][n]
  CS_EPI_HEAD_SCORE = 6,       // score[b][P*i+py][P*j+px] = act(acc + bias[n]), m=b*Np+i*gw+j, n=py*P+px
  // LayerNorm folded into the consuming projection (no separate LN pass over the fp32 residual stream):
  //   LN(x) W^T + b = rstd[m] * (fp16(x) W'^T - mu[m] * s[n]) + c[n],  W' = W*gamma (per input column), s[n] = sum_k W'[n][k],
  //   c[n] = b[n] + sum_k beta[k] W[n][k];  mu / rstd come from per-row partial sums the PRODUCING epilogue wrote.
  CS_EPI_LN_F16 = 7,          // out_f16 = rstd*(acc - mu*s) + c
  CS_EPI_LN_GELU_F16 = 8,     // ... then GELU
  CS_EPI_RESID_F32_LN = 9,     // CS_EPI_RESID_F32 + fp16 copy of the new rows + their partial (sum, sum of squares)
};

struct CsGemmParams {
  const h16_t* A;    // [M][lda] fp16, K contiguous
  const h16_t* W;    // [N][ldw] fp16, K contiguous (nn.Linear layout)
  int lda, ldw;
  int M, N, K;        // K % 64 == 0
  const float* bias;  // [N] or null
  const float* scale; // [N] or null
  const float* resid; // [M][ldr] fp32 or null
  int ldr;
  void* out;          // fp16 or fp32, see epilogue
  int ldc;
  // CS_EPI_PATCH_F32 / CS_EPI_HEAD_SCORE extras
  const float* pos;   // [(1+Np)][ldc] position table (patch)
  int bpc;            // persistent blocks per CU to launch (0 = 2, the number that is resident)
  const float* pmean; // patch epilogue: [M][4] per-row channel means removed by im2col (nullptr: none), added back as pmean . wsum
  const float* wsum;  // [3][ldc] fp32 sums of the patch weights over each channel's P*P taps
  int Np;             // patches per image
  int gw;             // patch-grid width
  int P;              // patch size (head)
  int act;            // 0 sigmoid, 1 tanh
  float powp;         // 1 -> identity
  // CS_EPI_HEAD_SCORE: the per-image mean of the score map in the same launch (score_summariser.py:180-192); all three or none.
  float* mean_part;     // [M][4 x column tiles] fp32 scratch: per patch row, the sum of one wave's columns (any contents on entry)
  unsigned* mean_cnt;   // [M / Np] arrival counters, ZERO on entry; the wave that completes an image's count sums its partials in a fixed
                        // order, writes the mean and puts the counter back to zero
  float* mean_out;      // [M / Np] fp32
  // LayerNorm fold (see CS_EPI_LN_*): producer side (RESID_F32_LN, PATCH_F32) ...
  h16_t* out_f16;    // [rows][ldc] fp16 copy of the fp32 rows written (the next GEMM's A operand), or null
  float* stats_out;    // [rows][stats_sp][2] partial (sum, sumsq) per row: slot = column_tile*4 + wave, or null
  int stats_sp;        //   128-row kernel (gemm.hip): 4 x its column tiles (192 / 128 wide); 256-tile kernel (gemm256.hip, LN = 2): N / 64
  // ... consumer side (LN_BF16, LN_GELU_BF16); `bias` carries c[n]
  const float* ln_part;  // 128-row kernel: [M][ln_sp][2] partial sums of the A rows (fp32 values before fp16 rounding), ln_sp in {4, 8, 16};
  int ln_sp;             // 256-tile kernel (LN = 1): ln_sp == 1 and ln_part = FINALISED rows [ceil(M / 256) * 256][2] = (mean, rstd) from
                         // cs_ln_finalize_launch -- whole 256-row tiles are fetched, so the buffer must hold the padded row count
  const float* col_s;    // [N] s[n]
  float ln_eps;
  int ablate;         // debug timing builds only (CS_ABLATE); 0 in the product
  int bf16;           // operand type of A, W and of a 16-bit output: 0 IEEE half, 1 bfloat16
};

struct CsAttnParams {
  const h16_t* Q; const h16_t* K; const h16_t* V; h16_t* O;
  int ldq, ldk, ldv, ldo;                              // row strides (elements)
  long long q_bs, k_bs, v_bs, o_bs;                    // batch strides (elements)
  int Lq, Lk, heads;
  int nbatch;                                          // filled by the launcher
  float scale_log2e;                                   // (1/sqrt(dh)) * log2(e)
  float* lse;                                          // optional [batch][heads][Lq]: m*ln2-scaled log-sum-exp (base 2)
  int bf16;                                            // operand type of Q, K, V, P and O: 0 IEEE half, 1 bfloat16
};

// Attention backward (attnbwd.hip): the forward's operands, dO and the lse cs_attn_kernel wrote; dQ, dK, dV in the operand type.
struct CsAttnBwdParams {
  const h16_t* Q; const h16_t* K; const h16_t* V; const h16_t* O; const h16_t* dO;
  const float* lse;                                    // [batch][heads][Lq], base 2
  int ldq, ldk, ldv, ldo, lddo;                        // row strides (elements)
  long long q_bs, k_bs, v_bs, o_bs, do_bs;             // batch strides (elements)
  int nbatch, heads, Lq, Lk;
  float scale_log2e;                                   // as CsAttnParams::scale_log2e
  h16_t* dQ; int lddq; long long dq_bs;
  h16_t* dK; int lddk; long long dk_bs;
  h16_t* dV; int lddv; long long dv_bs;
  float* D;                                            // workspace [batch][heads][Lq]: sum_d dO O per query row
  int bf16;
};

// Reference use (refuse.hip): Q / K / lse as the last decoder layer's cross-attention saw and wrote them; keys are N segments
// of Np rows.  Outputs (any may be null): share, peak_prob, peak_index (batch, N, Lq), entropy (batch, Lq).
struct CsRefUseParams {
  const h16_t* Q; const h16_t* K;
  int ldq, ldk;                                        // row strides (elements)
  long long q_bs, k_bs;                                // batch strides (elements)
  int Lq, N, Np, heads, nbatch;
  float scale_log2e;                                   // as CsAttnParams::scale_log2e
  const float* lse;                                    // [batch][heads][Lq], base 2, from cs_attn_kernel
  float* share; float* peak_prob; int32_t* peak_index; float* entropy;
  int bf16;                                            // operand type of Q and K
};

// One-pass input stage (SURVEY.md 8f-4 as worded: uint8 in, tokens out).  Filter tables of one resize geometry (preprocess.hip) and the per-image
// descriptor the patch kernel reads (patch.hip); images of one launch may differ in source size and geometry, not in the H x W window they produce.
struct CsU8Tables {
  const int *xmin, *xsize, *ymin, *ysize;  // per resized column / row: first source tap, number of taps
  const float *wx, *wy;                    // [rs_w][taps_x], [rs_h][taps_y] normalised triangle weights
  int taps_x, taps_y;
};
struct CsU8Desc {
  const uint8_t* data;  // device HWC RGB; null = the all-zero placeholder image (nvs_dataset.py:459-470: zeros BEFORE T.Normalize)
  CsU8Tables t;
  int row_bytes, crop_y, crop_x, pad_;
};

// Grouped reference selection (select.hip): what the host resolves per query -- the first bank row of its group, the group's rows, the row of
// the (G, C) centres it is centred with.  Checked on the host, uploaded with the call, clamped again where the device reads it.
struct CsSelTriple { int start, len, centre; };

// Preview sheet (sheet.hip): a panel as the kernel takes it, checked and translated from the public cs_sheet_panel by
// cs_op_sheet_compose (kind: the public CS_SHEET_* values), and the block of them that travels as one kernel argument.
struct CsSheetPanel {
  const uint8_t* src;         // IMAGE, BLEND: uint8 HWC RGB, rows row_bytes apart; RAMP: the 256 x 3 table
  const uint8_t* src2;        // BLEND: the second image, sh x sw as the first, rows row_bytes2 apart
  unsigned long long glyphs;  // TEXT: the glyph index of character i in bits [4 i, 4 i + 4)
  int kind, y, x, h, w;       // the destination rectangle, inside the canvas
  int sh, sw, row_bytes, row_bytes2;
  uint32_t rgb;               // r | g << 8 | b << 16
  int param;                  // FRAME: thickness; TEXT: scale
};
struct CsSheetPanels { CsSheetPanel p[48]; };  // (CS_SHEET_MAX_PANELS: 48 x 72 bytes, inside the 4 KiB a kernel's arguments may take)

// Encoder "token panel" kernel (panel.hip): one launch per DINOv2 layer does, for 128-row panels of the residual stream,
//   x += attn_o Wo'^T + bo'                 (attention output projection, LayerScale folded; HF modeling_dinov2.py:249-252,365-370)
//   x += GELU(LN2(x) W1'^T + b1') W2'^T + b2'   (norm2 + MLP + LayerScale; HF:373-378, 293-297)
//   u_out = fp16((x - mean) * rstd)         (norm1 of the NEXT layer without gamma/beta: they are folded into its QKV projection)
// The weights arrive as one pre-packed stream of 24-KiB "units" in the exact LDS image / consumption order (cs_panel_pack_*).
struct CsPanelParams {
  float* x;                // [M][C] fp32 residual stream, updated in place
  const h16_t* attn_o;    // [M][C] fp16 attention output, or null: no out-projection (x is taken as is)
  const h16_t* img;       // unit stream: [12 Wo units (if attn_o)] [96 MLP units]
  const float* bo;         // [C] out-projection bias (LayerScale folded), used when attn_o
  const float* b1;         // [4C] fc1 bias with LN2 beta folded in
  const float* b2;         // [C] fc2 bias (LayerScale folded)
  h16_t* u_out;           // [M][C] or null
  int M;
  float eps;               // LayerNorm eps (1e-6 in DINOv2)
  int bf16;                // operand type of attn_o, img, the hidden slices and u_out: 0 IEEE half, 1 bfloat16
};

// Decoder linear + residual + LayerNorm in one launch (rowln.hip): out = LN(resid + A W^T + bias), K = N = C
struct CsRowLnParams {
  const h16_t* A; int lda;      // [M][lda] 16-bit activations, K = C contiguous
  const h16_t* W; int ldw;      // [C][ldw] 16-bit weights (nn.Linear layout)
  const float* bias;            // [C]
  const float* resid; int ldr;  // [M][ldr] fp32 or null (no short cut)
  const float* gamma; const float* beta; float eps;
  float* out_f32; h16_t* out_f16;  // [M][C] each (out_f32 may alias resid: a lane reads exactly the elements it writes)
  int M;
  // optional second stage: out2 = act2(LN rows (16-bit) x W2^T + bias2), n2 a multiple of C (the sub-block's NEXT linear: the cross-attention's
  // Q projection, linear1 + ReLU, the next layer's packed QKV projection, the head's first linear + LeakyReLU); n2 = 0: none
  const h16_t* W2; int ldw2;    // [n2][ldw2]
  const float* bias2;           // [n2]
  h16_t* out2; int ld2;         // [M][ld2]
  int n2, act2;                 // act2: 0 none, 1 ReLU, 2 LeakyReLU(0.01)
};

// Head fit (headfit.hip).  The tile sizes are here because the tests read them through cs_head_fit_row_tile / _row_chunk.
#define CS_HEADFIT_ROW_TILE 64    // rows of one workgroup of head_grad_z / head_da
#define CS_HEADFIT_ROW_CHUNK 512  // rows of one fp32 partial of gemm_tn
#define CS_HEADFIT_NPAD 224       // columns of g: 196 padded to whole 32-deep k steps
struct CsHeadGradZ {
  const h16_t* A; int lda;      // [M][lda] hidden rows, M = B gh gw
  const h16_t* Wb; int ldw;     // [P*P][ldw] the head's second linear (nn.Linear layout)
  const float* bb;              // [P*P]
  const float* gt;              // [B][gh P][gw P] fp32
  int B, gh, gw, P, C, act; float powp;
  h16_t* g; int ldg;            // [M][ldg], ldg >= CS_HEADFIT_NPAD: 224 columns are written, the last 28 as zeros
  double* loss; double loss_scale; int loss_accumulate;  // *loss = (accumulate ? *loss : 0) + scale * sum |s - gt|
  float* colsum_part;           // [row tiles][CS_HEADFIT_NPAD] per-workgroup column sums of the rounded g, or null
  float* s_tap;                 // [M][P*P] fp32 s as the kernel formed it (cs_debug_op_head_grad_z_tap), or null
};
struct CsGemmTn {
  const h16_t* G; int ldg;      // [M][ldg], N columns used
  const h16_t* X; int ldx;      // [M][ldx], K columns used
  int M, N, K; float scale; int accumulate;
  float* out; int ldo;          // [N][ldo] fp32
  float* colsum;                // [N] scale * column sums of G by the same rule, or null
};
struct CsHeadBackward {
  const h16_t* X; int ldx; const h16_t* A; int lda; const h16_t* Wb; int ldw; const float* bb; const float* gt;
  int B, gh, gw, P, C, act; float powp; double inv_count; int accumulate;
  float *dWa, *dba, *dWb, *dbb; double* loss;
};

// Tail fit (tailfit.hip): the last decoder layer's linear1 -> ReLU -> linear2 -> + residual -> norm3 in front of the head.
#define CS_TAILFIT_LN_ROW_TILE 32  // rows of one workgroup of ln_backward (8 waves x 4 rows, or 4 x 8 for C > 512) = rows of one fp32 partial of d gamma / d beta
struct CsLnBackward {
  const float* y; int ldy;      // [M][ldy] fp32 rows the LayerNorm normalised
  const float* dx; int ldx;     // [M][ldx] fp32 gradient of the LayerNorm's output
  const float* gamma; float eps;
  int M, C; float scale; int accumulate;
  h16_t* dyh; int ldd;          // [M][ldd] gradient of y, rounded once to the operand type
  float *dgamma, *dbeta;        // [C] each: (accumulate ? old : 0) + scale * (sum_m dx * xhat | sum_m dx)
};
struct CsTailBackward {
  const float* x2;              // [M][C] fp32, contiguous: the last layer's norm2 output
  const h16_t* H; int ldh;      // [M][ldh] relu(linear1(x2)) as the forward stored it
  const h16_t* W2; int ldw2; const float* b2; const float* gamma3; float eps;  // linear2 (packed) and norm3's weight
  const h16_t* Wa; int ldwa;    // the head's first linear (packed)
  CsHeadBackward head;          // X, A, Wb, bb, gt, shapes, inv_count, accumulate, the head's four gradients and the loss
  float *dW1, *db1, *dW2, *db2, *dg3, *db3;
};

// Cross-attention fit (crossfit.hip): the last decoder layer's in_proj -> attention -> out_proj -> + residual -> norm2 in front of the tail.
struct CsCrossBackward {
  CsTailBackward tail;          // x2, H, the tail's weights, the head's block (B, gh, gw, C, inv_count, accumulate), the ten gradients and the loss
  const float* x1;              // [M][C] fp32, contiguous: the rows that entered the cross-attention block
  const h16_t* Qp; int ldq;     // [M][ldq] the query projection as the forward stored it (log2(e) / sqrt(dh) folded in)
  const h16_t* K; const h16_t* V; int ldkv;  // [Mk][ldkv] the layer's column blocks of the packed K | V rows, Mk = M N
  const h16_t* O; int ldo;      // [M][ldo] the attention output
  const float* lse;             // [B][heads][Np], base 2, as cs_attn_kernel wrote it
  const h16_t* mem; int ldm;    // [Mk][ldm] the reference tokens the K / V projection read
  const h16_t* W1; int ldw1; const h16_t* Wo; int ldwo; const float* bo; const float* gamma2;  // linear1 and out_proj (packed), norm2's weight
  int N, heads, short_cut;
  float *dWin, *dbin, *dWo, *dbo, *dg2, *db2;  // in_proj (3C, C) and (3C), out_proj (C, C) and (C), norm2 (C) each
};

// Whole-layer fit (layerfit.hip): the last decoder layer's self-attention -> out_proj -> + residual -> norm1 in front of the cross-attention fit.
struct CsLayerBackward {
  CsCrossBackward cross;        // x1, the cross-attention's operands and weights, the tail's and the head's blocks, the sixteen gradients and the loss
  const float* x0;              // [M][C] fp32, contiguous: the rows that entered the layer
  const h16_t* Qs; const h16_t* Ks; const h16_t* Vs; int ldqkv;  // [M][ldqkv] the column blocks of the packed projection rows (Qs' has log2(e) / sqrt(dh) folded in)
  const h16_t* Os; int ldos;    // [M][ldos] the self-attention's output
  const float* lse_s;           // [B][heads][Np], base 2, as cs_attn_kernel wrote it
  const h16_t* Wq; int ldwq;    // the cross-attention's packed query projection (log2(e) / sqrt(dh) folded in)
  const h16_t* Wo_s; int ldwos; const float* bo_s; const float* gamma1;  // the self-attention's out_proj (packed), norm1's weight
  float *dWin_s, *dbin_s, *dWo_s, *dbo_s, *dg1, *db1;  // in_proj (3C, C) and (3C), out_proj (C, C) and (C), norm1 (C) each
};

// ---- The launch surface between the kernel files and the host files (api.hip, forward.hip, ops.hip, fit_host.hip): every cs_*_launch / cs_*_check /
// cs_*_supported / size helper that one .hip defines and another calls, declared ONCE.  Every defining file includes this header, so a changed
// parameter list fails to compile there instead of linking (most of these are extern "C") and misbehaving at run time. ----

// patch.hip (C++ linkage)
size_t cs_patch_pack_elems(int C);
hipError_t cs_patch_pack_launch(const float* w, int C, h16_t* out, int bf, hipStream_t st);
int cs_patch_fused_supported(int H, int W, int P, int C);
hipError_t cs_patch_fused_u8_launch(const CsU8Desc* descs, int nq, int N, int img0, int I, int H, int W, int C, int row_span, const float* mean3,
                                    const float* std3, const h16_t* wfrag, const float* bias, const float* pos, const float* wsum, float* x, int bf,
                                    hipStream_t st);
int cs_patch_u8_runs(int W, int row_span);
hipError_t cs_patch_fused_launch(const float* xq, const float* xr, int N, int img0, int I, int H, int W, int C, const h16_t* wfrag,
                                 const float* bias, const float* pos, const float* wsum, float* x, int bf, hipStream_t st);

extern "C" {
// gemm.hip, gemm256.hip
int cs_gemm_column_tiles(int N);
const char* cs_gemm_check(const CsGemmParams* p, int epi);
hipError_t cs_gemm_launch(const CsGemmParams* p, int epi, hipStream_t stream);
int cs_gemm256_supported(const CsGemmParams* p, int epi);  // the shapes cs_gemm_launch routes to the 256-tile kernel
hipError_t cs_gemm256_launch(const CsGemmParams* p, int epi, int bf16, hipStream_t st);
extern int g_gemm_grid;  // cs_debug_gemm_grid: > 0 replaces the CU-derived block count of both GEMM launchers (before their clamps); 0 = off
// attention.hip
const char* cs_attn_check(const CsAttnParams* p, int dh, int batch);
hipError_t cs_attn_launch(const CsAttnParams* p, int dh, int batch, hipStream_t stream);
// attnbwd.hip
int cs_attnbwd_supported(int dh);
size_t cs_attnbwd_workspace(int batch, int heads, int Lq);
const char* cs_attnbwd_check(const CsAttnBwdParams* p);
hipError_t cs_attnbwd_launch(const CsAttnBwdParams* p, int dh, hipStream_t st);
// refuse.hip
const char* cs_refuse_check(const CsRefUseParams* p, int dh);
hipError_t cs_refuse_launch(const CsRefUseParams* p, int dh, hipStream_t stream);
// elementwise.hip
hipError_t cs_im2col_launch(const float* q, const float* refs, int N, int img0, h16_t* out, int I, int H, int W, int P, int Kp,
                            float* pmean, int bf, hipStream_t st);
hipError_t cs_patch_wsum_launch(const float* w, int C, int P, float* wsum, hipStream_t st);
hipError_t cs_ln_finalize_launch(const float* part, int M, int rows_padded, int sp, int C, float eps, float* stat, hipStream_t st);
hipError_t cs_layernorm_launch(const float* x, int M, int C, const float* g, const float* b, float eps, float* of32, h16_t* obf,
                               int bf, hipStream_t st);
hipError_t cs_final_ln_split_launch(const float* x, int I, int img0, int Np, int C, int N, const float* g, const float* b, float eps,
                                    const float* pe, float* q_f32, h16_t* q_bf, h16_t* mem_bf, int bf, hipStream_t st);
hipError_t cs_cls_rows_launch(float* x, int I, int T, int C, const float* cls, const float* pos, h16_t* xb, float* stats, int sp,
                              int bf, hipStream_t st);
hipError_t cs_ln_fold_consts_launch(const h16_t* wp, int ldp, const float* w, const float* beta, const float* bias, int N, int K,
                                    float* s_out, float* c_out, int bf, hipStream_t st);
hipError_t cs_pos_bicubic_launch(const float* pos, int G, int C, int gh, int gw, float grow, float* out, hipStream_t st);
hipError_t cs_pe_bilinear_launch(const float* pe, int ph, int pw, int C, int gh, int gw, float* out, hipStream_t st);
hipError_t cs_pe_interp_launch(const float* pe, int ph, int pw, int C, int gh, int gw, int mode, float* out, hipStream_t st);
hipError_t cs_pack_f16_launch(const float* w, int rows, int K, h16_t* out, int ldo, const float* row_scale, const float* col_scale,
                              int bf, hipStream_t st);
hipError_t cs_score_check_launch(const float* score, size_t n, unsigned* counter, hipStream_t st);
hipError_t cs_silu_mul_launch(h16_t* x, int M, int F, int ld, int bf, hipStream_t st);
hipError_t cs_vec_mul_launch(const float* a, const float* b, float* out, int n, hipStream_t st);
hipError_t cs_spin_launch(unsigned long long ticks, int blocks, int lds_bytes, hipStream_t st);
hipError_t cs_attn_weights_launch(const CsAttnParams* p, int dh, int batch, int head, float* out, hipStream_t st);
// preprocess.hip
hipError_t cs_preprocess_tables(int in_h, int in_w, int rs_h, int rs_w, int crop_y, int gh, int P, CsU8Tables* out, int* row_span, unsigned* generation);
void cs_preprocess_tables_hold(int on);
hipError_t cs_score_gray16_launch(const float* score, size_t n, int signed_range, uint16_t* out, hipStream_t stream);
hipError_t cs_score_rgb_launch(const float* score, size_t n, float vmin, float vmax, const uint8_t* lut, uint8_t* out, hipStream_t stream);
hipError_t cs_preprocess_launch(const uint8_t* img, int in_h, int in_w, int row_bytes, int rs_h, int rs_w, int crop_y, int crop_x, int oh,
                                int ow, const float* mean, const float* stdv, float* out, float* scratch, hipStream_t stream);
hipError_t cs_metric_map_launch(const uint16_t* maps, int B, int in_h, int in_w, int row_elems, int mode, int rs_h, int rs_w, int crop_y,
                                int crop_x, int oh, int ow, float* out, float* scratch, hipStream_t stream);
int cs_score_gt_slabs(size_t hw);
hipError_t cs_score_gt_stats_launch(const float* score, const float* gt, int B, size_t hw, double* scratch, double* stats, hipStream_t stream);
// panel.hip (eight waves) and panel4.hip (the four-wave form of the same kernel, its own weight image)
int cs_panel_supported(int C, int mlp_ratio);
size_t cs_panel8_image_bytes(int with_outproj);
hipError_t cs_panel_pack_launch(const float* wo, const float* ls1, const float* w1, const float* g2, const float* w2, const float* ls2,
                                h16_t* img, int bf16, hipStream_t st);
const char* cs_panel_check(const CsPanelParams* p);
hipError_t cs_panel_launch(const CsPanelParams* p, hipStream_t st);
size_t cs_panel4_image_bytes(int with_outproj);
hipError_t cs_panel4_pack_launch(const float* wo, const float* ls1, const float* w1, const float* g2, const float* w2, const float* ls2,
                                 h16_t* img, int bf16, hipStream_t st);
hipError_t cs_panel4_launch(const CsPanelParams* p, hipStream_t st);
// rowln.hip
int cs_rowln_supported(int C);
const char* cs_rowln_check(const CsRowLnParams* p, int C);
hipError_t cs_rowln_launch(const CsRowLnParams* p, int C, int bf16, hipStream_t st);
// png.hip
int cs_png_size_supported(int H, int W);
size_t cs_png_bound_bytes(int kind, int H, int W);
size_t cs_png_staging_bytes(int kind, int I, int H, int W);
hipError_t cs_png_encode_launch(const void* pixels, int kind, int I, int H, int W, long long image_stride, uint8_t* out, size_t slot_bytes,
                                uint32_t* lengths, void* workspace, int flags, hipStream_t st);
hipError_t cs_denorm_rgb8_launch(const float* chw, int I, int H, int W, const float* mean3, const float* std3, uint8_t* out, hipStream_t st);
// pngdec.hip
size_t cs_pngdec_workspace(int kind, int I, int H, int W, size_t total_file_bytes);
hipError_t cs_pngdec_launch(const uint8_t* files, const unsigned long long* file_offsets, const uint32_t* file_lengths, const uint32_t* spans,
                            const uint32_t* span_offsets, size_t files_bytes, int I, int kind, int H, int W, void* pixels, long long image_stride,
                            uint32_t* status, void* workspace, hipStream_t st);
// jpegdec.hip (flags: CS_JPEG_PROGRESSIVE adds jpegprog.hip's entropy launch and its workspace; levels: its schedule, 1 unless a test says 0)
size_t cs_jpgdec_workspace(int I, int H, int W, int flags);
hipError_t cs_jpgdec_launch(const uint8_t* files, const unsigned long long* file_offsets, const uint32_t* file_lengths, size_t files_bytes, int I,
                            int H, int W, void* pixels, long long image_stride, uint32_t* status, void* workspace, int flags, int levels,
                            hipStream_t st);
// gtmap.hip
int cs_gtmap_max_side();
hipError_t cs_gtmap_launch(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride, int kind, uint16_t* out,
                           int out_ld, hipStream_t st);
hipError_t cs_gtsums_launch(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride, uint64_t* sums, hipStream_t st);
// select.hip
hipError_t cs_token_descriptors_launch(const h16_t* tok, int I, int Np, int C, int bf, float* mean, hipStream_t st);
hipError_t cs_centre_launch(const float* mean, const int32_t* offsets, int G, int R, int C, float* centre, hipStream_t st);
hipError_t cs_bank_unit_launch(const float* mean, const int32_t* offsets, int G, int rows, int R, int C, const float* centre, float* unit, hipStream_t st);
hipError_t cs_query_unit_launch(const float* mean, int B, int C, const CsSelTriple* trip, int R, int G, const float* centre, float* unit, hipStream_t st);
hipError_t cs_similarity_launch(const float* q, int B, const float* bank, int R, int G, int C, const CsSelTriple* trip, int S, float* sim, hipStream_t st);
hipError_t cs_topn_launch(const float* sim, int B, int S, int R, int G, const CsSelTriple* trip, const int32_t* exclude, int N, int32_t* index, hipStream_t st);
hipError_t cs_gather_tokens_launch(const h16_t* bank, int R, int Np, int C, const int32_t* index, int slots, int blank, h16_t* out, hipStream_t st);
// gtsum.hip
hipError_t cs_metric_map_sums_launch(const uint16_t* ssim, const uint16_t* mae, int B, int H, int W, int row_elems, long long image_stride,
                                     uint64_t* sums, hipStream_t st);
// scorepool.hip
size_t cs_scorepool_workspace(int B, int H, int W);
hipError_t cs_scorepool_launch(const void* map, int is_f32, int B, int H, int W, int row_elems, long long image_stride, int signed_range,
                               const uint32_t* ranks, int Q, int S, uint64_t* sum, uint32_t* quant, uint64_t* tail, uint64_t* window,
                               void* scratch, hipStream_t st);
// sheet.hip
hipError_t cs_sheet_launch(const CsSheetPanels* panels, int n, uint8_t* canvas, int ch, int cw, hipStream_t st);
// headfit.hip (workspaces: 256-byte aligned device memory of the size the matching helper reports; the three whole backwards' are carved in
// fit_shared.h, each beginning with the one before: the launches leave dpre, dyh and dH there for the next scope)
int cs_headfit_supported(int C, int P);
size_t cs_head_grad_z_workspace(int M);
size_t cs_gemm_tn_workspace(int M, int N, int K);
size_t cs_head_backward_workspace(int M, int C);
hipError_t cs_head_grad_z_launch(const CsHeadGradZ* p, void* ws, int bf, hipStream_t st);
hipError_t cs_gemm_tn_launch(const CsGemmTn* p, void* ws, int bf, hipStream_t st);
hipError_t cs_head_backward_launch(const CsHeadBackward* p, void* ws, int bf, hipStream_t st);
// out (cols, ldo) = src (rows, lds)^T in 16 bits, zeros in the columns [rows, ldo)
hipError_t cs_transpose16_launch(const h16_t* src, int lds, int rows, int cols, h16_t* out, int ldo, hipStream_t st);
// tailfit.hip
size_t cs_ln_backward_workspace(int M, int C);
size_t cs_tail_backward_workspace(int M, int C);
hipError_t cs_ln_backward_launch(const CsLnBackward* p, void* ws, int bf, hipStream_t st);
hipError_t cs_tail_backward_launch(const CsTailBackward* p, void* ws, int bf, hipStream_t st);
// crossfit.hip
size_t cs_cross_backward_workspace(int B, int Np, int N, int C, int heads);
void cs_cross_backward_attn_params(const CsCrossBackward* p, void* ws, int bf, CsAttnBwdParams* out);  // the attention backward it queues
hipError_t cs_cross_backward_launch(const CsCrossBackward* p, void* ws, int bf, hipStream_t st);
// layerfit.hip
size_t cs_layer_backward_workspace(int B, int Np, int N, int C, int heads);
void cs_layer_backward_attn_params(const CsLayerBackward* p, void* ws, int bf, CsAttnBwdParams* out);  // the self-attention backward it queues
hipError_t cs_layer_backward_launch(const CsLayerBackward* p, void* ws, int bf, hipStream_t st);
hipError_t cs_adamw_launch(float* p, float* m, float* v, const float* g, long long n, float lr, float beta1, float beta2, float eps, float wd,
                           int step, h16_t* p16, int bf, hipStream_t st);
}
