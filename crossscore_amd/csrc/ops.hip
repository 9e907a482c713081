// Single-op entry points of the C ABI (cs_op_*): each kernel of the forward on its own, for the op-level tests and the measurement tools, and
// the PNG, ground-truth-map and score helpers the predict / evaluate drivers call.  Host-side only: argument checks, then one launch.
#include "cs_model.h"
#include "jpeg_probe.h"
#include "png_probe.h"
#include "sheet_font.h"

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

extern "C" {

// out_f32 / out_f16 (M, C) = LayerNorm(resid + A (M, C) W (C, C)^T + bias): the decoder's sub-block closing as the forward runs it (C = 384);
// with W2 the sub-block's next linear behind it: out2 (M, n2) = act2(LN rows (rounded to the operand type) x W2 (n2, C)^T + bias2)
static int rowln_op(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, const float* gamma, const float* beta, float eps,
                    float* out_f32, uint16_t* out_f16, const uint16_t* W2, const float* bias2, int n2, int act2, uint16_t* out2, int M, int C,
                    cs_stream stream) {
  CsRowLnParams q{};
  q.A = A; q.lda = C; q.W = W; q.ldw = C; q.bias = bias; q.resid = resid; q.ldr = C; q.gamma = gamma; q.beta = beta; q.eps = eps;
  q.out_f32 = out_f32; q.out_f16 = out_f16; q.M = M;
  q.W2 = W2; q.ldw2 = C; q.bias2 = bias2; q.out2 = out2; q.ld2 = n2; q.n2 = n2; q.act2 = act2;
  if (const char* e = cs_rowln_check(&q, C)) return fail(CS_ERR_BAD_ARG, "%s", e);
  HIPCHK(cs_rowln_launch(&q, C, g_op_bf16, (hipStream_t)stream));
  return 0;
}

int cs_op_linear_layernorm(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, const float* gamma, const float* beta,
                           float eps, float* out_f32, uint16_t* out_f16, int M, int C, cs_stream stream) {
  return rowln_op(A, W, bias, resid, gamma, beta, eps, out_f32, out_f16, nullptr, nullptr, 0, 0, nullptr, M, C, stream);
}

int cs_op_linear_layernorm_linear(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, const float* gamma,
                                  const float* beta, float eps, float* out_f32, uint16_t* out_f16, const uint16_t* W2, const float* bias2,
                                  int n2, int act2, uint16_t* out2, int M, int C, cs_stream stream) {
  if (n2 <= 0) return fail(CS_ERR_BAD_ARG, "linear + LayerNorm + linear: n2 must be positive");
  return rowln_op(A, W, bias, resid, gamma, beta, eps, out_f32, out_f16, W2, bias2, n2, act2, out2, M, C, stream);
}

int cs_op_gemm(const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K, const float* bias,
               const float* resid, int ldr, void* out, int ldc, int epi, const float* pos, int Np, int gw, int P, int act,
               float powp, uint16_t* out_f16, float* stats_out, int stats_sp, const float* ln_part, int ln_sp, const float* col_s,
               float ln_eps, cs_stream stream) {
  CsGemmParams g = gp(A, lda, W, ldw, M, N, K, bias, out, ldc);
  g.out_f16 = out_f16; g.stats_out = stats_out; g.stats_sp = stats_sp; g.ln_part = ln_part; g.ln_sp = ln_sp; g.col_s = col_s;
  g.ln_eps = ln_eps;
  g.resid = resid; g.ldr = ldr; g.pos = pos; g.Np = Np; g.gw = gw; g.P = P; g.act = act; g.powp = powp;
  g.bf16 = g_op_bf16;
  if (epi < 0 || epi > CS_EPI_RESID_F32_LN) return fail(CS_ERR_BAD_ARG, "gemm: unknown epilogue %d", epi);
  if (const char* e = cs_gemm_check(&g, epi)) return fail(CS_ERR_BAD_ARG, "%s", e);
  HIPCHK(cs_gemm_launch(&g, epi, (hipStream_t)stream));
  return 0;
}

int cs_op_head_score(const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int K, const float* bias, float* score, int Np, int gw, int P,
                     int act, float powp, float* mean_part, unsigned* mean_cnt, float* mean_out, cs_stream stream) {
  CsGemmParams g = gp(A, lda, W, ldw, M, P * P, K, bias, score, 4);
  g.Np = Np; g.gw = gw; g.P = P; g.act = act; g.powp = powp;
  g.mean_part = mean_part; g.mean_cnt = mean_cnt; g.mean_out = mean_out;
  g.bf16 = g_op_bf16;
  if (const char* e = cs_gemm_check(&g, CS_EPI_HEAD_SCORE)) return fail(CS_ERR_BAD_ARG, "%s", e);
  HIPCHK(cs_gemm_launch(&g, CS_EPI_HEAD_SCORE, (hipStream_t)stream));
  return 0;
}

int cs_op_attention(const uint16_t* Q, const uint16_t* K, const uint16_t* V, uint16_t* O, int ldq, int ldk, int ldv, int ldo,
                    long long q_bs, long long k_bs, long long v_bs, long long o_bs, int batch, int heads, int Lq, int Lk, int dh,
                    float q_scale, float* lse, cs_stream stream) {
  CsAttnParams a{};
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs; a.Lq = Lq; a.Lk = Lk; a.heads = heads;
  if (!(q_scale >= 0.f)) return fail(CS_ERR_BAD_ARG, "attention: q_scale must be >= 0 (0 = log2(e)/sqrt(dh))");
  a.scale_log2e = q_scale == 0.f ? LOG2E / std::sqrt((float)dh) : q_scale; a.lse = lse;
  a.bf16 = g_op_bf16;
  if (const char* e = cs_attn_check(&a, dh, batch)) return fail(CS_ERR_BAD_ARG, "%s", e);
  HIPCHK(cs_attn_launch(&a, dh, batch, (hipStream_t)stream));
  return 0;
}

int cs_op_attention_weights(const uint16_t* Q, const uint16_t* K, int ldq, int ldk, long long q_bs, long long k_bs, int batch,
                            int heads, int Lq, int Lk, int dh, float q_scale, const float* lse, int head, float* out, cs_stream stream) {
  if (!Q || !K || !lse || !out || !supported_dh(dh) || !(q_scale >= 0.f) || head < 0 || head >= heads || Lq <= 0 || Lk <= 0 || Lq > 65535 || batch <= 0 || batch > 65535)
    return fail(CS_ERR_BAD_ARG, "attention_weights: bad arguments");
  // the kernel reads Q and K rows in 16-byte chunks, like cs_attn_kernel: what cs_attn_check refuses for Q and K is refused here
  if (ldq % 8 || ldk % 8) return fail(CS_ERR_BAD_ARG, "attention_weights: row strides must keep 16-byte rows");
  if (q_bs % 8 || k_bs % 8) return fail(CS_ERR_BAD_ARG, "attention_weights: batch strides must keep 16-byte rows");
  if ((long long)Lk * ldk >= (1ll << 30)) return fail(CS_ERR_BAD_ARG, "attention_weights: Lk * row stride must stay below 2^30 elements");
  CsAttnParams a{};
  a.Q = Q; a.K = K; a.ldq = ldq; a.ldk = ldk; a.q_bs = q_bs; a.k_bs = k_bs; a.Lq = Lq; a.Lk = Lk; a.heads = heads;
  a.scale_log2e = q_scale == 0.f ? LOG2E / std::sqrt((float)dh) : q_scale; a.lse = const_cast<float*>(lse);
  a.bf16 = g_op_bf16;
  HIPCHK(cs_attn_weights_launch(&a, dh, batch, head, out, (hipStream_t)stream));
  return 0;
}

int cs_op_reference_use(const uint16_t* Q, const uint16_t* K, int ldq, int ldk, long long q_bs, long long k_bs, int batch, int heads, int Lq, int N,
                        int Np, int dh, float q_scale, const float* lse, float* share, float* peak_prob, int32_t* peak_index, float* entropy,
                        cs_stream stream) {
  if (!supported_dh(dh)) return fail(CS_ERR_UNSUPPORTED, "reference_use: head dim %d is none of 16, 48, 64, 96, 128, 192", dh);
  if (!(q_scale >= 0.f)) return fail(CS_ERR_BAD_ARG, "reference_use: q_scale must be >= 0 (0 = log2(e)/sqrt(dh))");
  CsRefUseParams a{};
  a.Q = Q; a.K = K; a.ldq = ldq; a.ldk = ldk; a.q_bs = q_bs; a.k_bs = k_bs; a.Lq = Lq; a.N = N; a.Np = Np; a.heads = heads; a.nbatch = batch;
  a.scale_log2e = q_scale == 0.f ? LOG2E / std::sqrt((float)dh) : q_scale; a.lse = lse;
  a.share = share; a.peak_prob = peak_prob; a.peak_index = peak_index; a.entropy = entropy;
  a.bf16 = g_op_bf16;
  if (const char* e = cs_refuse_check(&a, dh)) return fail(CS_ERR_BAD_ARG, "%s", e);
  if (!share && !peak_prob && !peak_index && !entropy) return 0;  // nothing asked for
  HIPCHK(cs_refuse_launch(&a, dh, (hipStream_t)stream));
  return 0;
}

int cs_op_layernorm(const float* x, int M, int C, const float* gamma, const float* beta, float eps, float* out_f32,
                    uint16_t* out_f16, cs_stream stream) {
  if (!x || !gamma || !beta || M <= 0 || C <= 0 || C % 4 || C > 2048) return fail(CS_ERR_BAD_ARG, "layernorm: C must be a multiple of 4 and <= 2048");
  HIPCHK(cs_layernorm_launch(x, M, C, gamma, beta, eps, out_f32, out_f16, g_op_bf16, (hipStream_t)stream));
  return 0;
}

// the SwiGLU gate exactly as the forward launches it (swiglu layers): in place on M rows `ld` apart, x[m][j] = silu(x[m][j]) * x[m][F + j], j < F
int cs_op_silu_mul(uint16_t* x, int M, int F, int ld, cs_stream stream) {
  if (!x || M <= 0 || F <= 0 || F % 8 || ld < 2 * F || ld % 8) return fail(CS_ERR_BAD_ARG, "silu_mul: F and ld must be multiples of 8, ld >= 2 F");
  HIPCHK(cs_silu_mul_launch(x, M, F, ld, g_op_bf16, (hipStream_t)stream));
  return 0;
}

int cs_op_ln_finalize(const float* part, int M, int rows_padded, int sp, int C, float eps, float* stat, cs_stream stream) {
  if (!part || !stat || M <= 0 || rows_padded < M || sp <= 0 || C <= 0) return fail(CS_ERR_BAD_ARG, "ln_finalize: bad arguments");
  HIPCHK(cs_ln_finalize_launch(part, M, rows_padded, sp, C, eps, stat, (hipStream_t)stream));
  return 0;
}

int cs_op_im2col(const float* x, uint16_t* out, int I, int H, int W, int P, int Kp, cs_stream stream) {
  if (!x || !out || I <= 0 || P <= 0 || H < P || W < P || Kp % 8 || Kp < 3 * P * P) return fail(CS_ERR_BAD_ARG, "im2col: bad arguments");
  HIPCHK(cs_im2col_launch(x, nullptr, 0, 0, out, I, H, W, P, Kp, nullptr, g_op_bf16, (hipStream_t)stream));
  return 0;
}

// Patch embedding in one launch (patch.hip), as the forward runs it for 14-pixel patches and C = 384 n.  Same arguments and result as
// cs_op_patch_embed(centred = 1); CS_ERR_BAD_ARG for shapes the one-launch form does not take.
int cs_op_patch_embed_fused(const float* x, const float* w, const float* bias, const float* pos, int I, int H, int W, int P, int C,
                            float* out, cs_stream stream) {
  if (!x || !w || !bias || !pos || !out || I <= 0 || !cs_patch_fused_supported(H, W, P, C)) return fail(CS_ERR_BAD_ARG, "patch_embed_fused: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  h16_t* wf = nullptr; float* wsum = nullptr;
  HIPCHK(hipMalloc(&wf, cs_patch_pack_elems(C) * sizeof(h16_t)));
  HIPCHK(hipMalloc(&wsum, (size_t)3 * C * sizeof(float)));
  int rc = 0;
  auto chk = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(CS_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
  chk(cs_patch_pack_launch(w, C, wf, g_op_bf16, st), "pack");
  chk(cs_patch_wsum_launch(w, C, P, wsum, st), "wsum");
  if (!rc) chk(cs_patch_fused_launch(x, nullptr, 0, 0, I, H, W, C, wf, bias, pos, wsum, out, g_op_bf16, st), "patch");
  chk(hipStreamSynchronize(st), "sync");
  hipFree(wf); hipFree(wsum);
  return rc;
}

// The same launch fed from ONE decoded uint8 image geometry (test entry point of the one-pass input stage): imgs = I device images of identical
// size (I, in_h, row_bytes) -> out (I * (1 + Np), C) as cs_op_patch_embed_fused on cs_op_preprocess_u8's output of each image.
int cs_op_patch_embed_fused_u8(const uint8_t* imgs, int I, int in_h, int in_w, int row_bytes, int rs_h, int rs_w, int crop_y, int crop_x, int H, int W,
                               const float* mean3, const float* std3, const float* w, const float* bias, const float* pos, int P, int C, float* out,
                               cs_stream stream) {
  if (!imgs || !w || !bias || !pos || !out || !mean3 || !std3 || I <= 0 || !cs_patch_fused_supported(H, W, P, C) || crop_y < 0 || crop_x < 0 ||
      crop_y + H > rs_h || crop_x + W > rs_w || row_bytes < 3 * in_w)
    return fail(CS_ERR_BAD_ARG, "patch_embed_fused_u8: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  CsU8Tables t{};
  int span = 0;
  HIPCHK(cs_preprocess_tables(in_h, in_w, rs_h, rs_w, crop_y, H / P, P, &t, &span, nullptr));
  if (cs_patch_u8_runs(W, span) <= 0) return fail(CS_ERR_UNSUPPORTED, "patch_embed_fused_u8: %d source rows per patch row do not fit", span);
  std::vector<CsU8Desc> hd(I);
  for (int i = 0; i < I; ++i) { hd[i].data = imgs + (size_t)i * in_h * row_bytes; hd[i].t = t; hd[i].row_bytes = row_bytes; hd[i].crop_y = crop_y; hd[i].crop_x = crop_x; }
  h16_t* wf = nullptr; float* wsum = nullptr; CsU8Desc* dd = nullptr;
  HIPCHK(hipMalloc(&wf, cs_patch_pack_elems(C) * sizeof(h16_t)));
  HIPCHK(hipMalloc(&wsum, (size_t)3 * C * sizeof(float)));
  HIPCHK(hipMalloc(&dd, (size_t)I * sizeof(CsU8Desc)));
  int rc = 0;
  auto chk = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(CS_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
  chk(hipMemcpy(dd, hd.data(), (size_t)I * sizeof(CsU8Desc), hipMemcpyHostToDevice), "descriptors");
  chk(cs_patch_pack_launch(w, C, wf, g_op_bf16, st), "pack");
  chk(cs_patch_wsum_launch(w, C, P, wsum, st), "wsum");
  if (!rc) chk(cs_patch_fused_u8_launch(dd, I, 0, 0, I, H, W, C, span, mean3, std3, wf, bias, pos, wsum, out, g_op_bf16, st), "patch_u8");
  chk(hipStreamSynchronize(st), "sync");
  hipFree(wf); hipFree(wsum); hipFree(dd);
  return rc;
}

// Patch embedding as the forward ran it before patch.hip (im2col -> MFMA GEMM with the PATCH epilogue), for op-level tests of the mean-centred form:
// centred != 0: every patch's per-channel mean is removed before the fp16 rounding (im2col_rows_kernel) and added back in fp32 as
// mean_ch * sum_taps W[n][ch] by the epilogue (patch_wsum_kernel).  x (I,3,H,W), w (C,3,P,P), bias (C), pos ((1 + Np), C) -> out (I * (1 + Np), C)
// fp32 with the patch rows written (CLS rows untouched).  Allocates its temporaries: a test entry point, not a hot path.
int cs_op_patch_embed(const float* x, const float* w, const float* bias, const float* pos, int I, int H, int W, int P, int C, int centred,
                      float* out, cs_stream stream) {
  if (!x || !w || !bias || !pos || !out || I <= 0 || P != 14 || H < P || W < P || C <= 0 || C % 64) return fail(CS_ERR_BAD_ARG, "patch_embed: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int gh = H / P, gw = W / P, Np = gh * gw, Kp = ((3 * P * P + 63) / 64) * 64;
  h16_t *A = nullptr, *Wp = nullptr; float *pmean = nullptr, *wsum = nullptr;
  HIPCHK(hipMalloc(&A, (size_t)I * Np * Kp * sizeof(h16_t)));
  HIPCHK(hipMalloc(&Wp, (size_t)C * Kp * sizeof(h16_t)));
  HIPCHK(hipMalloc(&pmean, (size_t)I * Np * 4 * sizeof(float)));
  HIPCHK(hipMalloc(&wsum, (size_t)3 * C * sizeof(float)));
  int rc = 0;
  auto chk = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(CS_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
  chk(cs_pack_f16_launch(w, C, 3 * P * P, Wp, Kp, nullptr, nullptr, g_op_bf16, st), "pack");
  chk(cs_patch_wsum_launch(w, C, P, wsum, st), "wsum");
  chk(cs_im2col_launch(x, nullptr, 0, 0, A, I, H, W, P, Kp, centred ? pmean : nullptr, g_op_bf16, st), "im2col");
  if (!rc) {
    CsGemmParams g = gp(A, Kp, Wp, Kp, I * Np, C, Kp, bias, out, C);
    g.pos = pos; g.Np = Np; g.bf16 = g_op_bf16;
    if (centred) { g.pmean = pmean; g.wsum = wsum; }
    if (const char* e = cs_gemm_check(&g, CS_EPI_PATCH_F32)) rc = fail(CS_ERR_BAD_ARG, "%s", e);
    else chk(cs_gemm_launch(&g, CS_EPI_PATCH_F32, st), "gemm");
  }
  chk(hipStreamSynchronize(st), "sync");
  hipFree(A); hipFree(Wp); hipFree(pmean); hipFree(wsum);
  return rc;
}

int cs_op_preprocess_u8(const uint8_t* img, int in_h, int in_w, int in_row_bytes, int rs_h, int rs_w, int crop_y, int crop_x, int out_h,
                        int out_w, const float* mean3, const float* std3, float* out, float* scratch, cs_stream stream) {
  if (!img || !out || !mean3 || !std3 || in_h <= 0 || in_w <= 0 || in_row_bytes < 3 * in_w || rs_h <= 0 || rs_w <= 0 || out_h <= 0 ||
      out_w <= 0 || crop_y < 0 || crop_x < 0 || crop_y + out_h > rs_h || crop_x + out_w > rs_w)
    return fail(CS_ERR_BAD_ARG, "preprocess_u8: bad sizes (the crop window must lie inside the resized image)");
  if ((rs_h != in_h || rs_w != in_w) && !scratch) return fail(CS_ERR_BAD_ARG, "preprocess_u8: a resize needs in_h*rs_w*3 floats of scratch");
  for (int c = 0; c < 3; ++c)
    if (!(std3[c] > 0.f)) return fail(CS_ERR_BAD_ARG, "preprocess_u8: std must be positive");
  HIPCHK(cs_preprocess_launch(img, in_h, in_w, in_row_bytes, rs_h, rs_w, crop_y, crop_x, out_h, out_w, mean3, std3, out, scratch,
                              (hipStream_t)stream));
  return 0;
}

int cs_op_score_to_gray16(const float* score, long long n, int signed_range, uint16_t* out, cs_stream stream) {
  if (!score || !out || n <= 0 || (signed_range != 0 && signed_range != 1)) return fail(CS_ERR_BAD_ARG, "score_to_gray16: bad arguments");
  HIPCHK(cs_score_gray16_launch(score, (size_t)n, signed_range, out, (hipStream_t)stream));
  return 0;
}

int cs_op_metric_map_u16(const uint16_t* maps, int B, int in_h, int in_w, int in_row_elems, int mode, int rs_h, int rs_w, int crop_y,
                         int crop_x, int out_h, int out_w, float* out, float* scratch, cs_stream stream) {
  if (!out || B <= 0 || B > 1024 || in_h <= 0 || in_w <= 0 || in_row_elems < in_w || rs_h <= 0 || rs_w <= 0 || out_h <= 0 || out_w <= 0 ||
      crop_y < 0 || crop_x < 0 || crop_y + out_h > rs_h || crop_x + out_w > rs_w)
    return fail(CS_ERR_BAD_ARG, "metric_map_u16: bad sizes (1 <= B <= 1024; the crop window must lie inside the resized map)");
  if (mode < CS_METRIC_SSIM_M1_1 || mode > CS_METRIC_MSE) return fail(CS_ERR_BAD_ARG, "metric_map_u16: mode %d is none of CS_METRIC_*", mode);
  if (maps && (rs_h != in_h || rs_w != in_w) && !scratch)
    return fail(CS_ERR_BAD_ARG, "metric_map_u16: a resize needs B*in_h*rs_w floats of scratch");
  HIPCHK(cs_metric_map_launch(maps, B, in_h, in_w, in_row_elems, mode, rs_h, rs_w, crop_y, crop_x, out_h, out_w, out, scratch, (hipStream_t)stream));
  return 0;
}

int cs_op_gt_metric_map_u8(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride_bytes, int kind, uint16_t* out,
                           int out_row_elems, cs_stream stream) {
  if (kind != CS_GTMAP_SSIM && kind != CS_GTMAP_MAE) return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: kind %d is neither CS_GTMAP_SSIM nor CS_GTMAP_MAE", kind);
  if (B <= 0 || B > 1024 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: bad sizes (B %d, H %d, W %d; 1 <= B <= 1024)", B, H, W);
  if (H > cs_gtmap_max_side() || W > cs_gtmap_max_side())
    return fail(CS_ERR_UNSUPPORTED, "gt_metric_map_u8: %d x %d has a side above %d", H, W, cs_gtmap_max_side());
  if (image_stride_bytes < (long long)H * W * 3)
    return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: image stride %lld is below the image's %lld bytes", image_stride_bytes, (long long)H * W * 3);
  if (out_row_elems < W) return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: output row of %d samples is below the width %d", out_row_elems, W);
  if (!render || !gt || !out) return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: null pointer");
  if ((uintptr_t)out & 1) return fail(CS_ERR_BAD_ARG, "gt_metric_map_u8: 16-bit samples must be 2-byte aligned");
  HIPCHK(cs_gtmap_launch(render, gt, B, H, W, image_stride_bytes, kind, out, out_row_elems, (hipStream_t)stream));
  return 0;
}

int cs_op_metric_map_sums_u16(const uint16_t* ssim, const uint16_t* mae, int B, int H, int W, int row_elems, long long image_stride_elems,
                              uint64_t* sums, cs_stream stream) {
  if (B <= 0 || B > 1024 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: bad sizes (B %d, H %d, W %d; 1 <= B <= 1024)", B, H, W);
  if (H > cs_gtmap_max_side() || W > cs_gtmap_max_side())
    return fail(CS_ERR_UNSUPPORTED, "metric_map_sums_u16: %d x %d has a side above %d", H, W, cs_gtmap_max_side());
  if (row_elems < W) return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: row of %d samples is below the width %d", row_elems, W);
  if (image_stride_elems < (long long)(H - 1) * row_elems + W)
    return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: map stride %lld is below the map's %lld samples", image_stride_elems,
                (long long)(H - 1) * row_elems + W);
  if (!ssim || !mae || !sums) return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: null pointer");
  if (((uintptr_t)ssim | (uintptr_t)mae) & 1) return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: 16-bit samples must be 2-byte aligned");
  if ((uintptr_t)sums & 7) return fail(CS_ERR_BAD_ARG, "metric_map_sums_u16: the sums must be 8-byte aligned");
  HIPCHK(cs_metric_map_sums_launch(ssim, mae, B, H, W, row_elems, image_stride_elems, sums, (hipStream_t)stream));
  return 0;
}

int cs_op_gt_metric_sums_u8(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride_bytes, uint64_t* sums,
                            cs_stream stream) {
  if (B <= 0 || B > 1024 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "gt_metric_sums_u8: bad sizes (B %d, H %d, W %d; 1 <= B <= 1024)", B, H, W);
  if (H > cs_gtmap_max_side() || W > cs_gtmap_max_side())
    return fail(CS_ERR_UNSUPPORTED, "gt_metric_sums_u8: %d x %d has a side above %d", H, W, cs_gtmap_max_side());
  if (image_stride_bytes < (long long)H * W * 3)
    return fail(CS_ERR_BAD_ARG, "gt_metric_sums_u8: image stride %lld is below the image's %lld bytes", image_stride_bytes, (long long)H * W * 3);
  if (!render || !gt || !sums) return fail(CS_ERR_BAD_ARG, "gt_metric_sums_u8: null pointer");
  if ((uintptr_t)sums & 7) return fail(CS_ERR_BAD_ARG, "gt_metric_sums_u8: the sums must be 8-byte aligned");
  HIPCHK(cs_gtsums_launch(render, gt, B, H, W, image_stride_bytes, sums, (hipStream_t)stream));
  return 0;
}

size_t cs_score_gt_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * cs_score_gt_slabs((size_t)H * W) * 6 * sizeof(double);
}

int cs_op_score_gt_stats(const float* score, const float* gt, int B, int H, int W, double* stats, void* scratch, cs_stream stream) {
  if (!score || !gt || !stats || !scratch || B <= 0 || B > 65535 || H <= 0 || W <= 0)
    return fail(CS_ERR_BAD_ARG, "score_gt_stats: bad arguments");
  HIPCHK(cs_score_gt_stats_launch(score, gt, B, (size_t)H * W, (double*)scratch, stats, (hipStream_t)stream));
  return 0;
}

size_t cs_score_pool_workspace_bytes(int B, int H, int W, int Q) {
  if (B <= 0 || B > 1024 || H <= 0 || W <= 0 || H > 4096 || W > 4096 || Q < 1 || Q > 16) return 0;
  return cs_scorepool_workspace(B, H, W);
}

// the checks and rank arithmetic both entries share; map: fp32 scores (is_f32) or 16-bit codes
static int score_pool_op(const char* who, const void* map, int is_f32, int B, int H, int W, int row_elems, long long image_stride, int signed_range,
                         const int32_t* permille, int Q, int S, uint64_t* sum, uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch,
                         cs_stream stream) {
  if (B <= 0 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "%s: bad sizes (B %d, H %d, W %d)", who, B, H, W);
  if (B > 1024 || H > 4096 || W > 4096)
    return fail(CS_ERR_UNSUPPORTED, "%s: B %d, %d x %d is above 1024 images of 4096 x 4096", who, B, H, W);
  if (signed_range != 0 && signed_range != 1) return fail(CS_ERR_BAD_ARG, "%s: signed_range %d is neither 0 nor 1", who, signed_range);
  if (Q < 1 || Q > 16) return fail(CS_ERR_BAD_ARG, "%s: %d permille values (1 .. 16)", who, Q);
  if (!map || !permille || !sum || !quant || !tail || !scratch) return fail(CS_ERR_BAD_ARG, "%s: null pointer", who);
  for (int j = 0; j < Q; ++j)
    if (permille[j] < 0 || permille[j] > 1000) return fail(CS_ERR_BAD_ARG, "%s: permille[%d] = %d is outside 0 .. 1000", who, j, (int)permille[j]);
  if (S < 0 || S > 255 || S > H || S > W)
    return fail(CS_ERR_BAD_ARG, "%s: a window of %d does not lie inside %d x %d (1 .. min(H, W, 255); 0: none)", who, S, H, W);
  if (row_elems < W) return fail(CS_ERR_BAD_ARG, "%s: row of %d samples is below the width %d", who, row_elems, W);
  if (image_stride < (long long)(H - 1) * row_elems + W)
    return fail(CS_ERR_BAD_ARG, "%s: map stride %lld is below the map's %lld samples", who, image_stride, (long long)(H - 1) * row_elems + W);
  if ((uintptr_t)map & (is_f32 ? 3 : 1)) return fail(CS_ERR_BAD_ARG, "%s: the map is not aligned to its samples", who);
  if (((uintptr_t)sum | (uintptr_t)tail | (uintptr_t)window) & 7) return fail(CS_ERR_BAD_ARG, "%s: sum, tail and window must be 8-byte aligned", who);
  if ((uintptr_t)quant & 3) return fail(CS_ERR_BAD_ARG, "%s: quant must be 4-byte aligned", who);
  if ((uintptr_t)scratch & 15) return fail(CS_ERR_BAD_ARG, "%s: the scratch must be 16-byte aligned", who);
  const long long n = (long long)H * W;
  uint32_t ranks[32];
  for (int j = 0; j < Q; ++j) {
    const long long q = permille[j], k = q * n / 1000;
    ranks[j] = (uint32_t)(q * (n - 1) / 1000);       // the quantile's index into the sorted codes
    ranks[Q + j] = (uint32_t)((k < 1 ? 1 : k) - 1);  // the index of the last of the k smallest codes
  }
  HIPCHK(cs_scorepool_launch(map, is_f32, B, H, W, row_elems, image_stride, signed_range, ranks, Q, S, sum, quant, tail, window, scratch,
                             (hipStream_t)stream));
  return 0;
}

int cs_op_score_pool_f32(const float* score, int B, int H, int W, int signed_range, const int32_t* permille, int Q, int S, uint64_t* sum,
                         uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch, cs_stream stream) {
  return score_pool_op("score_pool_f32", score, 1, B, H, W, W, (long long)H * W, signed_range, permille, Q, S, sum, quant, tail, window, scratch, stream);
}

int cs_op_score_pool_u16(const uint16_t* codes, int B, int H, int W, int row_elems, long long image_stride_elems, const int32_t* permille, int Q,
                         int S, uint64_t* sum, uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch, cs_stream stream) {
  return score_pool_op("score_pool_u16", codes, 0, B, H, W, row_elems, image_stride_elems, 0, permille, Q, S, sum, quant, tail, window, scratch, stream);
}

// every check of the header's contract, then the panels in the kernel's form: one launch
int cs_op_sheet_compose(const cs_sheet_panel* panels, int n_panels, uint8_t* canvas, int canvas_h, int canvas_w, cs_stream stream) {
  static_assert(sizeof(CsSheetPanels) == CS_SHEET_MAX_PANELS * sizeof(CsSheetPanel) && sizeof(CsSheetPanels) + 64 <= 4096, "kernel arguments");
  const int kMax = CS_SHEET_MAX_SIDE;
  if (!canvas || canvas_h <= 0 || canvas_w <= 0 || n_panels < 0 || (n_panels > 0 && !panels))
    return fail(CS_ERR_BAD_ARG, "sheet_compose: bad arguments (canvas %d x %d, %d panels)", canvas_h, canvas_w, n_panels);
  if (n_panels > CS_SHEET_MAX_PANELS) return fail(CS_ERR_UNSUPPORTED, "sheet_compose: %d panels are more than %d", n_panels, CS_SHEET_MAX_PANELS);
  if (canvas_h > kMax || canvas_w > kMax) return fail(CS_ERR_UNSUPPORTED, "sheet_compose: a %d x %d canvas is above %d a side", canvas_h, canvas_w, kMax);
  CsSheetPanels dev{};
  for (int i = 0; i < n_panels; ++i) {
    const cs_sheet_panel& p = panels[i];
    CsSheetPanel& q = dev.p[i];
    if (p.kind < CS_SHEET_FILL || p.kind > CS_SHEET_TEXT) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has the unknown kind %d", i, p.kind);
    const bool image = p.kind == CS_SHEET_IMAGE || p.kind == CS_SHEET_BLEND;
    if (p.dst_h > kMax || p.dst_w > kMax || (image && (p.src_h > kMax || p.src_w > kMax)))
      return fail(CS_ERR_UNSUPPORTED, "sheet_compose: panel %d (%d x %d from %d x %d) has a side above %d", i, p.dst_h, p.dst_w, p.src_h, p.src_w, kMax);
    if (p.dst_h <= 0 || p.dst_w <= 0) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has the empty rectangle %d x %d", i, p.dst_h, p.dst_w);
    if (p.dst_y < 0 || p.dst_x < 0 || p.dst_y > canvas_h - p.dst_h || p.dst_x > canvas_w - p.dst_w)
      return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d (%d x %d at %d, %d) does not lie inside the %d x %d canvas", i, p.dst_h, p.dst_w, p.dst_y,
                  p.dst_x, canvas_h, canvas_w);
    q.kind = p.kind; q.y = p.dst_y; q.x = p.dst_x; q.h = p.dst_h; q.w = p.dst_w;
    q.rgb = (uint32_t)p.rgb[0] | (uint32_t)p.rgb[1] << 8 | (uint32_t)p.rgb[2] << 16;
    q.param = p.param;
    if (image) {
      if (!p.src || p.src_h <= 0 || p.src_w <= 0 || p.src_row_bytes < 3 * p.src_w)
        return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has no source, an empty one or rows of %d bytes below 3 x %d", i, p.src_row_bytes, p.src_w);
      q.src = p.src; q.sh = p.src_h; q.sw = p.src_w; q.row_bytes = p.src_row_bytes;
      if (p.kind == CS_SHEET_BLEND) {
        if (!p.src2 || p.src2_row_bytes < 3 * p.src2_w) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has no second source or too short rows", i);
        if (p.src2_h != p.src_h || p.src2_w != p.src_w)
          return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d blends %d x %d with %d x %d", i, p.src_h, p.src_w, p.src2_h, p.src2_w);
        q.src2 = p.src2; q.row_bytes2 = p.src2_row_bytes;
      }
    } else if (p.kind == CS_SHEET_RAMP) {
      if (!p.src) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has no colour table", i);
      q.src = p.src;
    } else if (p.kind == CS_SHEET_FRAME) {
      if (p.param < 1) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has the thickness %d", i, p.param);
    } else if (p.kind == CS_SHEET_TEXT) {
      int n = 0;
      while (n < 16 && p.text[n]) ++n;
      if (p.param < 1 || n < 1) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has the scale %d and %d characters", i, p.param, n);
      for (int k = 0; k < n; ++k) {
        const int g = sheet_glyph_index(p.text[k]);
        if (g < 0) return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d has a character (code %d) outside \"%s\"", i, (int)p.text[k], CS_SHEET_CHARS);
        q.glyphs |= (unsigned long long)g << (4 * k);
      }
      if (p.param > kMax || p.dst_h != 7 * p.param || p.dst_w != (6 * n - 1) * p.param)
        return fail(CS_ERR_BAD_ARG, "sheet_compose: panel %d: %d characters at scale %d take %d x %d, not %d x %d", i, n, p.param, 7 * p.param,
                    (6 * n - 1) * p.param, p.dst_h, p.dst_w);
    }
  }
  HIPCHK(cs_sheet_launch(&dev, n_panels, canvas, canvas_h, canvas_w, (hipStream_t)stream));
  return 0;
}

int cs_op_score_to_rgb(const float* score, long long n, float vmin, float vmax, const uint8_t* lut256x3, uint8_t* out, cs_stream stream) {
  if (!score || !out || !lut256x3 || n <= 0 || !(vmax > vmin)) return fail(CS_ERR_BAD_ARG, "score_to_rgb: bad arguments");
  HIPCHK(cs_score_rgb_launch(score, (size_t)n, vmin, vmax, lut256x3, out, (hipStream_t)stream));
  return 0;
}

size_t cs_png_bound(int kind, int H, int W) {
  if (H <= 0 || W <= 0 || !cs_png_size_supported(H, W)) return 0;
  return cs_png_bound_bytes(kind, H, W);
}

size_t cs_png_workspace_bytes(int kind, int I, int H, int W) {
  if (H <= 0 || W <= 0 || !cs_png_size_supported(H, W)) return 0;
  return cs_png_staging_bytes(kind, I, H, W);
}

int cs_op_png_encode_ex(const void* pixels, int kind, int I, int H, int W, long long image_stride_bytes, uint8_t* out, size_t slot_bytes,
                        uint32_t* lengths, void* workspace, cs_stream stream, int flags) {
  if (flags < 0 || flags > (CS_PNG_DYNAMIC | CS_PNG_ADAPTIVE_FILTER))
    return fail(CS_ERR_BAD_ARG, "png_encode: flags %d outside 0 .. 3 (CS_PNG_DYNAMIC | CS_PNG_ADAPTIVE_FILTER)", flags);
  if (kind != CS_PNG_GRAY16 && kind != CS_PNG_RGB8) return fail(CS_ERR_BAD_ARG, "png_encode: kind %d is neither CS_PNG_GRAY16 nor CS_PNG_RGB8", kind);
  if (I <= 0 || I > 65535 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "png_encode: bad sizes (I %d, H %d, W %d; 1 <= I <= 65535)", I, H, W);
  if (!cs_png_size_supported(H, W)) return fail(CS_ERR_UNSUPPORTED, "png_encode: %d x %d is larger than 4096 x 4096", H, W);
  const long long image_bytes = (long long)H * W * (kind == CS_PNG_GRAY16 ? 2 : 3);
  if (image_stride_bytes < image_bytes || (kind == CS_PNG_GRAY16 && (image_stride_bytes & 1)))
    return fail(CS_ERR_BAD_ARG, "png_encode: image stride %lld is below the image's %lld bytes (or odd for 16-bit samples)", image_stride_bytes, image_bytes);
  if (slot_bytes < cs_png_bound_bytes(kind, H, W))
    return fail(CS_ERR_BAD_ARG, "png_encode: slot of %zu bytes is below the bound %zu of this size", slot_bytes, cs_png_bound_bytes(kind, H, W));
  if (!pixels || !out || !lengths || !workspace) return fail(CS_ERR_BAD_ARG, "png_encode: null pointer");
  if (kind == CS_PNG_GRAY16 && ((uintptr_t)pixels & 1)) return fail(CS_ERR_BAD_ARG, "png_encode: 16-bit samples must be 2-byte aligned");
  if ((uintptr_t)workspace & 15) return fail(CS_ERR_BAD_ARG, "png_encode: the workspace must be 16-byte aligned");
  HIPCHK(cs_png_encode_launch(pixels, kind, I, H, W, image_stride_bytes, out, slot_bytes, lengths, workspace, flags, (hipStream_t)stream));
  return 0;
}

int cs_op_png_encode(const void* pixels, int kind, int I, int H, int W, long long image_stride_bytes, uint8_t* out, size_t slot_bytes,
                     uint32_t* lengths, void* workspace, cs_stream stream) {
  return cs_op_png_encode_ex(pixels, kind, I, H, W, image_stride_bytes, out, slot_bytes, lengths, workspace, stream, 0);
}

// ---- PNG decoder (pngdec.hip): the host probe (png_probe.h), the workspace size and the launch
int cs_png_probe(const uint8_t* file, size_t n, cs_png_info* info, cs_png_span* spans, int max_spans) {
  if (!file || !info || max_spans < 0) return fail(CS_ERR_BAD_ARG, "png_probe: null pointer");
  char why[256];
  const int rc = cs_png_probe_walk(file, n, info, spans, max_spans, why, sizeof why);
  return rc == CS_OK ? 0 : fail(rc, "%s", why);
}

size_t cs_png_decode_workspace_bytes(int kind, int I, int H, int W, size_t total_file_bytes) {
  if (H <= 0 || W <= 0 || I <= 0 || I > 65535 || !cs_png_size_supported(H, W)) return 0;
  return cs_pngdec_workspace(kind, I, H, W, total_file_bytes);
}

int cs_op_png_decode(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, const cs_png_span* spans,
                     const uint32_t* span_offsets, size_t total_file_bytes, int I, int kind, int H, int W, void* pixels, long long image_stride_bytes,
                     uint32_t* status, void* workspace, cs_stream stream) {
  if (kind != CS_PNG_GRAY16 && kind != CS_PNG_RGB8) return fail(CS_ERR_BAD_ARG, "png_decode: kind %d is neither CS_PNG_GRAY16 nor CS_PNG_RGB8", kind);
  if (I <= 0 || I > 65535 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "png_decode: bad sizes (I %d, H %d, W %d; 1 <= I <= 65535)", I, H, W);
  if (!cs_png_size_supported(H, W)) return fail(CS_ERR_UNSUPPORTED, "png_decode: %d x %d is larger than 4096 x 4096", H, W);
  const long long image_bytes = (long long)H * W * (kind == CS_PNG_GRAY16 ? 2 : 3);
  if (image_stride_bytes < image_bytes || (kind == CS_PNG_GRAY16 && (image_stride_bytes & 1)))
    return fail(CS_ERR_BAD_ARG, "png_decode: image stride %lld is below the image's %lld bytes (or odd for 16-bit samples)", image_stride_bytes, image_bytes);
  if (total_file_bytes == 0 || total_file_bytes >= ((size_t)1 << 40)) return fail(CS_ERR_BAD_ARG, "png_decode: %zu file bytes (1 .. 2^40 - 1)", total_file_bytes);
  if (!files || !file_offsets || !file_lengths || !spans || !span_offsets || !pixels || !status || !workspace) return fail(CS_ERR_BAD_ARG, "png_decode: null pointer");
  if (kind == CS_PNG_GRAY16 && ((uintptr_t)pixels & 1)) return fail(CS_ERR_BAD_ARG, "png_decode: 16-bit samples must be 2-byte aligned");
  if ((uintptr_t)workspace & 15) return fail(CS_ERR_BAD_ARG, "png_decode: the workspace must be 16-byte aligned");
  static_assert(sizeof(cs_png_span) == 8, "span layout");
  HIPCHK(cs_pngdec_launch(files, (const unsigned long long*)file_offsets, file_lengths, (const uint32_t*)spans, span_offsets, total_file_bytes, I, kind, H, W,
                          pixels, image_stride_bytes, status, workspace, (hipStream_t)stream));
  return 0;
}

// ---- JPEG decoder (jpegdec.hip): the host probe (jpeg_probe.h), the workspace size and the launches
static int jpeg_probe_result(int rc, const cs_jpeg_probe_result& r, const cs_jpeg_probe_scans& x, const char* why, cs_jpeg_info* info,
                             cs_jpeg_scan_info* scans) {
  info->width = r.width; info->height = r.height; info->components = r.components; info->sampling = r.sampling;
  info->restart_interval = r.restart_interval; info->entropy_offset = r.entropy_offset;
  if (scans) { scans->process = x.process; scans->scans = x.scans; scans->entropy_offset = x.entropy_offset; }
  if (rc != CS_JPEG_PROBE_OK) return fail(rc == CS_JPEG_PROBE_BAD_ARG ? CS_ERR_BAD_ARG : CS_ERR_UNSUPPORTED, "%s", why);
  return 0;
}

int cs_jpeg_probe(const uint8_t* file, size_t n, cs_jpeg_info* info) {
  if (!file || !info) return fail(CS_ERR_BAD_ARG, "jpeg_probe: null pointer");
  cs_jpeg_probe_result r;
  cs_jpeg_probe_scans x;
  char why[256];
  const int rc = cs_jpeg_probe_walk_ex(file, n, 0, &r, &x, why, sizeof why);
  return jpeg_probe_result(rc, r, x, why, info, nullptr);
}

int cs_jpeg_probe_ex(const uint8_t* file, size_t n, int flags, cs_jpeg_info* info, cs_jpeg_scan_info* scans) {
  if (!file || !info) return fail(CS_ERR_BAD_ARG, "jpeg_probe: null pointer");
  if (flags & ~CS_JPEG_PROGRESSIVE) return fail(CS_ERR_BAD_ARG, "jpeg_probe: unknown flags %d", flags);
  cs_jpeg_probe_result r;
  cs_jpeg_probe_scans x;
  char why[256];
  const int rc = cs_jpeg_probe_walk_ex(file, n, flags, &r, &x, why, sizeof why);
  return jpeg_probe_result(rc, r, x, why, info, scans);
}

size_t cs_jpeg_decode_workspace_bytes_ex(int I, int H, int W, size_t total_file_bytes, int flags) {
  if (H <= 0 || W <= 0 || I <= 0 || I > 65535 || total_file_bytes == 0 || !cs_png_size_supported(H, W) || (flags & ~CS_JPEG_PROGRESSIVE)) return 0;
  return cs_jpgdec_workspace(I, H, W, flags);
}

size_t cs_jpeg_decode_workspace_bytes(int I, int H, int W, size_t total_file_bytes) {
  return cs_jpeg_decode_workspace_bytes_ex(I, H, W, total_file_bytes, 0);
}

static int g_jpeg_scan_levels = 1;
void cs_debug_jpeg_scan_levels(int on) { g_jpeg_scan_levels = on ? 1 : 0; }

int cs_op_jpeg_decode_ex(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, size_t total_file_bytes, int I, int H,
                         int W, void* pixels, long long image_stride_bytes, uint32_t* status, void* workspace, int flags, cs_stream stream) {
  if (I <= 0 || I > 65535 || H <= 0 || W <= 0) return fail(CS_ERR_BAD_ARG, "jpeg_decode: bad sizes (I %d, H %d, W %d; 1 <= I <= 65535)", I, H, W);
  if (H > 4096 || W > 4096) return fail(CS_ERR_UNSUPPORTED, "jpeg_decode: %d x %d is larger than 4096 x 4096", H, W);
  if (flags & ~CS_JPEG_PROGRESSIVE) return fail(CS_ERR_BAD_ARG, "jpeg_decode: unknown flags %d", flags);
  const long long image_bytes = (long long)H * W * 3;
  if (image_stride_bytes < image_bytes) return fail(CS_ERR_BAD_ARG, "jpeg_decode: image stride %lld is below the image's %lld bytes", image_stride_bytes, image_bytes);
  if (total_file_bytes == 0 || total_file_bytes >= ((size_t)1 << 40)) return fail(CS_ERR_BAD_ARG, "jpeg_decode: %zu file bytes (1 .. 2^40 - 1)", total_file_bytes);
  if (!files || !file_offsets || !file_lengths || !pixels || !status || !workspace) return fail(CS_ERR_BAD_ARG, "jpeg_decode: null pointer");
  if ((uintptr_t)workspace & 15) return fail(CS_ERR_BAD_ARG, "jpeg_decode: the workspace must be 16-byte aligned");
  HIPCHK(cs_jpgdec_launch(files, (const unsigned long long*)file_offsets, file_lengths, total_file_bytes, I, H, W, pixels, image_stride_bytes, status,
                          workspace, flags, g_jpeg_scan_levels, (hipStream_t)stream));
  return 0;
}

int cs_op_jpeg_decode(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, size_t total_file_bytes, int I, int H,
                      int W, void* pixels, long long image_stride_bytes, uint32_t* status, void* workspace, cs_stream stream) {
  return cs_op_jpeg_decode_ex(files, file_offsets, file_lengths, total_file_bytes, I, H, W, pixels, image_stride_bytes, status, workspace, 0, stream);
}

int cs_op_denorm_to_rgb8(const float* chw, int I, int H, int W, const float* mean3, const float* std3, uint8_t* out, cs_stream stream) {
  if (!chw || !out || !mean3 || !std3 || I <= 0 || H <= 0 || W <= 0 || (long long)I * H * W > (1ll << 38))
    return fail(CS_ERR_BAD_ARG, "denorm_to_rgb8: bad arguments");
  HIPCHK(cs_denorm_rgb8_launch(chw, I, H, W, mean3, std3, out, (hipStream_t)stream));
  return 0;
}

int cs_op_pos_bicubic_ex(const float* pos, int G, int C, int gh, int gw, int legacy, float* out, cs_stream stream) {
  if (!pos || !out || G <= 0 || C <= 0 || gh <= 0 || gw <= 0) return fail(CS_ERR_BAD_ARG, "pos_bicubic: bad arguments");
  HIPCHK(cs_pos_bicubic_launch(pos, G, C, gh, gw, legacy ? 0.1f : 0.0f, out, (hipStream_t)stream));
  return 0;
}

int cs_op_pos_bicubic(const float* pos, int G, int C, int gh, int gw, float* out, cs_stream stream) {
  return cs_op_pos_bicubic_ex(pos, G, C, gh, gw, 0, out, stream);
}

int cs_op_pe_bilinear(const float* pe, int ph, int pw, int C, int gh, int gw, float* out, cs_stream stream) {
  if (!pe || !out || ph <= 0 || pw <= 0 || C <= 0 || gh <= 0 || gw <= 0) return fail(CS_ERR_BAD_ARG, "pe_bilinear: bad arguments");
  HIPCHK(cs_pe_bilinear_launch(pe, ph, pw, C, gh, gw, out, (hipStream_t)stream));
  return 0;
}

int cs_op_pe_interp(const float* pe, int ph, int pw, int C, int gh, int gw, int mode, float* out, cs_stream stream) {
  if (!pe || !out || ph <= 0 || pw <= 0 || C <= 0 || gh <= 0 || gw <= 0) return fail(CS_ERR_BAD_ARG, "cs_op_pe_interp: bad arguments");
  if (mode != 0 && mode != 1) return fail(CS_ERR_BAD_ARG, "cs_op_pe_interp: mode must be 0 (bilinear) or 1 (bicubic)");
  HIPCHK(cs_pe_interp_launch(pe, ph, pw, C, gh, gw, mode, out, (hipStream_t)stream));
  return 0;
}

int cs_op_streams_overlap(cs_stream a, cs_stream b, int* overlap) {
  if (!overlap || a == b) return fail(CS_ERR_BAD_ARG, "streams_overlap: two different streams and a result pointer are needed");
  bool yes = false;
  if (int r = streams_overlap((hipStream_t)a, (hipStream_t)b, &yes)) return r;
  *overlap = yes ? 1 : 0;
  return 0;
}

int cs_op_pack_f16(const float* w, int rows, int K, uint16_t* out, int ldo, const float* row_scale, const float* col_scale,
                    cs_stream stream) {
  if (!w || !out || rows <= 0 || K <= 0 || ldo < K) return fail(CS_ERR_BAD_ARG, "pack_f16: bad arguments");
  HIPCHK(cs_pack_f16_launch(w, rows, K, out, ldo, row_scale, col_scale, g_op_bf16, (hipStream_t)stream));
  return 0;
}

int cs_op_panel_pack(const float* wo, const float* ls1, const float* w1, const float* g2, const float* w2, const float* ls2,
                     uint16_t* img, cs_stream stream) {
  if (!w1 || !w2 || !img) return fail(CS_ERR_BAD_ARG, "panel_pack: null argument");
  if (g_panel_impl) HIPCHK(cs_panel4_pack_launch(wo, ls1, w1, g2, w2, ls2, img, g_op_bf16, (hipStream_t)stream));
  else HIPCHK(cs_panel_pack_launch(wo, ls1, w1, g2, w2, ls2, img, g_op_bf16, (hipStream_t)stream));
  return 0;
}


size_t cs_panel_image_bytes(int with_outproj) { return g_panel_impl ? cs_panel4_image_bytes(with_outproj) : cs_panel8_image_bytes(with_outproj); }

int cs_op_encoder_panel(float* x, const uint16_t* attn_o, const uint16_t* img, const float* bo, const float* b1, const float* b2,
                        uint16_t* u_out, int M, float eps, cs_stream stream) {
  CsPanelParams q{};
  q.x = x; q.attn_o = attn_o; q.img = img; q.bo = bo; q.b1 = b1; q.b2 = b2; q.u_out = u_out; q.M = M; q.eps = eps;
  q.bf16 = g_op_bf16;
  if (const char* e = cs_panel_check(&q)) return fail(CS_ERR_BAD_ARG, "%s", e);
  if (g_panel_impl) HIPCHK(cs_panel4_launch(&q, (hipStream_t)stream));
  else HIPCHK(cs_panel_launch(&q, (hipStream_t)stream));
  return 0;
}

int cs_op_ln_fold_consts(const uint16_t* w_packed, int ldp, const float* w, const float* beta, const float* bias, int N, int K,
                         float* s_out, float* c_out, cs_stream stream) {
  if (!w || !beta || !c_out || (w_packed && (!s_out || ldp < K)) || N <= 0 || K <= 0) return fail(CS_ERR_BAD_ARG, "ln_fold_consts: bad arguments");
  HIPCHK(cs_ln_fold_consts_launch(w_packed, ldp, w, beta, bias, N, K, s_out, c_out, g_op_bf16, (hipStream_t)stream));
  return 0;
}

// ---- reference selection by similarity (select.hip) ----
int cs_op_token_descriptors(const uint16_t* tokens, int I, int Np, int C, int dtype, float* mean_out, cs_stream stream) {
  if (!tokens || !mean_out || I <= 0 || Np <= 0 || C <= 0) return fail(CS_ERR_BAD_ARG, "token_descriptors: bad arguments");
  if (dtype != CS_DTYPE_F16 && dtype != CS_DTYPE_BF16) return fail(CS_ERR_BAD_ARG, "token_descriptors: dtype must be CS_DTYPE_F16 or CS_DTYPE_BF16");
  if (C % 64 || I > 65535) return fail(CS_ERR_UNSUPPORTED, "token_descriptors: C must be a multiple of 64 and I <= 65535");
  HIPCHK(cs_token_descriptors_launch(tokens, I, Np, C, dtype == CS_DTYPE_BF16, mean_out, (hipStream_t)stream));
  return 0;
}

int cs_op_descriptor_centre(const float* mean, int R, int C, float* centre_out, cs_stream stream) {
  if (!mean || !centre_out || R <= 0 || C <= 0) return fail(CS_ERR_BAD_ARG, "descriptor_centre: bad arguments");
  if (C % 64) return fail(CS_ERR_UNSUPPORTED, "descriptor_centre: C must be a multiple of 64");
  HIPCHK(cs_centre_launch(mean, nullptr, 1, R, C, centre_out, (hipStream_t)stream));
  return 0;
}

int cs_op_descriptor_unit(const float* mean, int I, int C, const float* centre, float* unit_out, cs_stream stream) {
  if (!mean || !centre || !unit_out || I <= 0 || C <= 0) return fail(CS_ERR_BAD_ARG, "descriptor_unit: bad arguments");
  HIPCHK(cs_bank_unit_launch(mean, nullptr, 1, I, I, C, centre, unit_out, (hipStream_t)stream));
  return 0;
}

int cs_op_select_references(const float* q_unit, int B, const float* bank_unit, int R, int C, const int32_t* exclude, int N, int32_t* index_out,
                            float* sim_out, cs_stream stream) {
  if (!q_unit || !bank_unit || !index_out || !sim_out) return fail(CS_ERR_BAD_ARG, "select_references: null tensor");
  if (int r = select_check(B, R, C, N, false, exclude != nullptr)) return r;
  HIPCHK(cs_similarity_launch(q_unit, B, bank_unit, R, 1, C, nullptr, R, sim_out, (hipStream_t)stream));
  HIPCHK(cs_topn_launch(sim_out, B, R, R, 1, nullptr, exclude, N, index_out, (hipStream_t)stream));
  return 0;
}

int cs_op_gather_tokens_ex(const uint16_t* bank, int R, int Np, int C, const int32_t* index, int B, int N, uint16_t* out, cs_stream stream,
                           int blank_row) {
  if (!bank || !index || !out || R <= 0 || Np <= 0 || C <= 0 || B <= 0 || N <= 0) return fail(CS_ERR_BAD_ARG, "gather_tokens: bad arguments");
  if (blank_row < -1 || blank_row >= R) return fail(CS_ERR_BAD_ARG, "gather_tokens: blank_row = %d outside [-1, %d)", blank_row, R);
  if (((long long)Np * C) % 8 || (long long)B * N > 65535) return fail(CS_ERR_UNSUPPORTED, "gather_tokens: Np * C must be a multiple of 8 and B * N <= 65535");
  HIPCHK(cs_gather_tokens_launch(bank, R, Np, C, index, B * N, blank_row, out, (hipStream_t)stream));
  return 0;
}

int cs_op_gather_tokens(const uint16_t* bank, int R, int Np, int C, const int32_t* index, int B, int N, uint16_t* out, cs_stream stream) {
  return cs_op_gather_tokens_ex(bank, R, Np, C, index, B, N, out, stream, -1);
}

// The grouped forms have no handle and no workspace: the host arrays they resolve travel through a process-wide ring whose slots own the device
// side of the copy and the kernels' scratch (StageRing).  Every check comes first: a refused call has queued nothing.
namespace {
std::mutex g_stage_mutex;
StageRing g_stage;

// `bytes` of src -> the head of a slot's device memory of bytes (rounded up to 256) + scratch_bytes, asynchronously on st
int stage_upload(const void* src, size_t bytes, size_t scratch_bytes, hipStream_t st, StageRing::Slot** sl) {
  if (int r = stage_take(g_stage, bytes, ((bytes + 255) & ~size_t(255)) + scratch_bytes, sl)) return r;
  memcpy((*sl)->host, src, bytes);
  HIPCHK(hipMemcpyAsync((*sl)->dev, (*sl)->host, bytes, hipMemcpyHostToDevice, st));
  return 0;
}
// behind the last kernel that reads the slot's device memory
int stage_done(StageRing::Slot* sl, hipStream_t st) {
  HIPCHK(hipEventRecord(sl->ev, st));
  sl->used = true;
  return 0;
}
}  // namespace

int cs_op_group_descriptors(const float* mean, int R, int C, const int32_t* offsets, int G, float* centre_out, float* unit_out, cs_stream stream) {
  if (!mean || !centre_out || !unit_out || R <= 0 || C <= 0) return fail(CS_ERR_BAD_ARG, "group_descriptors: bad arguments");
  if (C % 64 || R > 65536) return fail(CS_ERR_UNSUPPORTED, "group_descriptors: C must be a multiple of 64 and R <= 65536");
  if (int r = group_offsets_check(offsets, G, R, nullptr)) return r;
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(g_stage_mutex);
  StageRing::Slot* sl = nullptr;
  if (int r = stage_upload(offsets, (size_t)(G + 1) * sizeof(int32_t), 0, st, &sl)) return r;
  const int32_t* d_off = static_cast<const int32_t*>(sl->dev);
  HIPCHK(cs_centre_launch(mean, d_off, G, R, C, centre_out, st));
  HIPCHK(cs_bank_unit_launch(mean, d_off, G, offsets[G], R, C, centre_out, unit_out, st));
  return stage_done(sl, st);
}

int cs_op_select_references_grouped(const float* q_mean, int B, const int32_t* query_group, const float* bank_unit, const float* centre,
                                    const int32_t* offsets, int G, int R, int C, const int32_t* exclude, int N, int32_t* index_out, float* sim_out,
                                    cs_stream stream) {
  if (!q_mean || !bank_unit || !centre || !index_out || !sim_out) return fail(CS_ERR_BAD_ARG, "select_references_grouped: null tensor");
  if (int r = select_check(B, R, C, N, true, false)) return r;
  int S = 0;
  if (int r = group_offsets_check(offsets, G, R, &S)) return r;
  if (int r = query_groups_check(query_group, B, G)) return r;
  std::vector<CsSelTriple> trip((size_t)B);
  fill_triples(query_group, B, offsets, trip.data());
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(g_stage_mutex);
  StageRing::Slot* sl = nullptr;
  const size_t tb = (size_t)B * sizeof(CsSelTriple);
  if (int r = stage_upload(trip.data(), tb, (size_t)B * C * sizeof(float), st, &sl)) return r;
  const CsSelTriple* t = static_cast<const CsSelTriple*>(sl->dev);
  float* q_unit = reinterpret_cast<float*>(static_cast<char*>(sl->dev) + ((tb + 255) & ~size_t(255)));  // the queries' units: scratch
  HIPCHK(cs_query_unit_launch(q_mean, B, C, t, R, G, centre, q_unit, st));
  HIPCHK(cs_similarity_launch(q_unit, B, bank_unit, R, G, C, t, S, sim_out, st));
  HIPCHK(cs_topn_launch(sim_out, B, S, R, G, t, exclude, N, index_out, st));
  return stage_done(sl, st);
}

}  // extern "C"
