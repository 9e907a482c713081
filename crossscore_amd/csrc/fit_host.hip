// The host side of fitting on the device, no kernels: for each of the nested scopes head, tail, cross and layer the checks,
// the cs_op_* operator, the *_supported and *_workspace_bytes queries, and -- at the end of the file -- the backwards on a handle, which read what
// its last forward kept through the carve the forward wrote it through (cs_fit::kept_carve).  Every check comes first: a refused call has queued nothing.
#include "cs_model.h"

#include <cmath>
#include <initializer_list>

extern "C" {

// ---- head fit (headfit.hip): checks first, then the launches ----
int cs_head_fit_supported(int hidden, int patch) { return cs_headfit_supported(hidden, patch); }
int cs_head_fit_row_tile(void) { return CS_HEADFIT_ROW_TILE; }
int cs_head_fit_row_chunk(void) { return CS_HEADFIT_ROW_CHUNK; }
int cs_head_fit_g_columns(void) { return CS_HEADFIT_NPAD; }

size_t cs_head_backward_workspace_bytes(int M, int C, int P) {
  if (M <= 0 || !cs_headfit_supported(C, P)) return 0;
  return cs_head_backward_workspace(M, C);
}

size_t cs_gemm_tn_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return cs_gemm_tn_workspace(M, N, K);
}

static bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// what every head-fit entry asks of the head's shape and of the 16-bit operands A (M, C) and Wb (P P, C)
static int head_fit_shape_check(const char* op, const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B,
                                int gh, int gw, int P, int C, int act, float powp, const void* ws) {
  if (!A || !Wb || !bb || !gt || !ws) return fail(CS_ERR_BAD_ARG, "%s: null pointer", op);
  if (B <= 0 || gh <= 0 || gw <= 0) return fail(CS_ERR_BAD_ARG, "%s: empty batch or patch grid", op);
  if (!cs_headfit_supported(C, P)) return fail(CS_ERR_UNSUPPORTED, "%s: built for hidden a multiple of 64 in [64, 4096] and patch 14 (hidden %d, patch %d)", op, C, P);
  if (act != 0 && act != 1) return fail(CS_ERR_BAD_ARG, "%s: act must be 0 (sigmoid) or 1 (tanh)", op);
  if (!(powp > 0.f)) return fail(CS_ERR_BAD_ARG, "%s: power factor must be positive", op);
  // (the reference forces p = 1 with tanh, regression_layer.py:48-56: a power of a negative base has no gradient worth defining)
  if (act == 1 && powp != 1.0f) return fail(CS_ERR_UNSUPPORTED, "%s: tanh with a power factor other than 1 is not built", op);
  if ((long long)B * gh * gw > (1ll << 22)) return fail(CS_ERR_UNSUPPORTED, "%s: more than 2^22 token rows; split the batch", op);
  if (lda < C || ldw < C || lda % 8 || ldw % 8) return fail(CS_ERR_BAD_ARG, "%s: row strides must be multiples of 8 elements and at least C", op);
  if (misaligned(A, 16) || misaligned(Wb, 16) || misaligned(bb, 4) || misaligned(gt, 4) || misaligned(ws, 256))
    return fail(CS_ERR_BAD_ARG, "%s: misaligned pointer (16-bit operands 16 bytes, fp32 4, workspace 256)", op);
  return 0;
}

static int head_grad_z_op(const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P, int C,
                          int act, float powp, uint16_t* g, int ldg, double* loss_sum, float* colsum_part, float* s_tap, void* ws, cs_stream stream) {
  if (int r = head_fit_shape_check("head_grad_z", A, lda, Wb, ldw, bb, gt, B, gh, gw, P, C, act, powp, ws)) return r;
  if (!g || !loss_sum) return fail(CS_ERR_BAD_ARG, "head_grad_z: null pointer");
  if (ldg < CS_HEADFIT_NPAD || ldg % 8 || misaligned(g, 16) || misaligned(loss_sum, 8) || misaligned(colsum_part, 4))
    return fail(CS_ERR_BAD_ARG, "head_grad_z: g needs rows of at least %d elements, a multiple of 8 apart, 16-byte aligned; the loss 8-byte aligned", CS_HEADFIT_NPAD);
  CsHeadGradZ z{};
  z.A = A; z.lda = lda; z.Wb = Wb; z.ldw = ldw; z.bb = bb; z.gt = gt; z.B = B; z.gh = gh; z.gw = gw; z.P = P; z.C = C; z.act = act; z.powp = powp;
  z.g = g; z.ldg = ldg; z.loss = loss_sum; z.loss_scale = 1.0; z.loss_accumulate = 1; z.colsum_part = colsum_part; z.s_tap = s_tap;
  HIPCHK(cs_head_grad_z_launch(&z, ws, g_op_bf16, (hipStream_t)stream));
  return 0;
}

int cs_op_head_grad_z(const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P, int C,
                      int act, float powp, uint16_t* g, int ldg, double* loss_sum, float* colsum_part, void* ws, cs_stream stream) {
  return head_grad_z_op(A, lda, Wb, ldw, bb, gt, B, gh, gw, P, C, act, powp, g, ldg, loss_sum, colsum_part, nullptr, ws, stream);
}

// tests: the same call with s (M, P P) fp32 as the epilogue formed it
int cs_debug_op_head_grad_z_tap(const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                                int C, int act, float powp, uint16_t* g, int ldg, double* loss_sum, float* colsum_part, float* s_out, void* ws,
                                cs_stream stream) {
  if (!s_out || misaligned(s_out, 4)) return fail(CS_ERR_BAD_ARG, "head_grad_z tap: s_out missing or misaligned");
  return head_grad_z_op(A, lda, Wb, ldw, bb, gt, B, gh, gw, P, C, act, powp, g, ldg, loss_sum, colsum_part, s_out, ws, stream);
}

int cs_op_gemm_tn(const uint16_t* G, int ldg, const uint16_t* X, int ldx, int M, int N, int K, float scale, int accumulate, float* out, int ldo,
                  float* colsum, void* ws, cs_stream stream) {
  if (!G || !X || !out || !ws) return fail(CS_ERR_BAD_ARG, "gemm_tn: null pointer");
  if (M <= 0 || N <= 0 || K <= 0) return fail(CS_ERR_BAD_ARG, "gemm_tn: empty shape");
  if (K % 8 || N > 65535 * 64 || (long long)M > (1ll << 22) || (long long)N * K >= (1ll << 31))
    return fail(CS_ERR_UNSUPPORTED, "gemm_tn: K must be a multiple of 8, M <= 2^22, N K < 2^31 (M %d, N %d, K %d)", M, N, K);
  if (ldg < N || ldx < K || ldo < K || ldg % 8 || ldx % 8) return fail(CS_ERR_BAD_ARG, "gemm_tn: row strides must cover the rows; those of G and X must be multiples of 8 elements");
  if (misaligned(G, 16) || misaligned(X, 16) || misaligned(out, 4) || misaligned(colsum, 4) || misaligned(ws, 256))
    return fail(CS_ERR_BAD_ARG, "gemm_tn: misaligned pointer (16-bit operands 16 bytes, fp32 4, workspace 256)");
  CsGemmTn t{};
  t.G = G; t.ldg = ldg; t.X = X; t.ldx = ldx; t.M = M; t.N = N; t.K = K; t.scale = scale; t.accumulate = accumulate != 0; t.out = out; t.ldo = ldo;
  t.colsum = colsum;
  HIPCHK(cs_gemm_tn_launch(&t, ws, g_op_bf16, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

// cs_op_head_backward and cs_head_backward come through here
int cs_host::head_backward_run(const char* op, const CsHeadBackward& q, void* ws, int bf, hipStream_t st) {
  if (int r = head_fit_shape_check(op, q.A, q.lda, q.Wb, q.ldw, q.bb, q.gt, q.B, q.gh, q.gw, q.P, q.C, q.act, q.powp, ws)) return r;
  if (!q.X || !q.dWa || !q.dba || !q.dWb || !q.dbb || !q.loss) return fail(CS_ERR_BAD_ARG, "%s: null pointer", op);
  if (q.ldx < q.C || q.ldx % 8 || misaligned(q.X, 16)) return fail(CS_ERR_BAD_ARG, "%s: X needs 16-byte aligned rows a multiple of 8 elements apart", op);
  if (misaligned(q.dWa, 4) || misaligned(q.dba, 4) || misaligned(q.dWb, 4) || misaligned(q.dbb, 4) || misaligned(q.loss, 8))
    return fail(CS_ERR_BAD_ARG, "%s: misaligned output", op);
  if (!(q.inv_count > 0.0)) return fail(CS_ERR_BAD_ARG, "%s: inv_count must be positive", op);
  HIPCHK(cs_head_backward_launch(&q, ws, bf, st));
  return 0;
}

extern "C" {

int cs_op_head_backward(const uint16_t* X, int ldx, const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B,
                        int gh, int gw, int P, int C, int act, float powp, double inv_count, int accumulate, float* dWa, float* dba, float* dWb,
                        float* dbb, double* loss, void* ws, cs_stream stream) {
  CsHeadBackward q{};
  q.X = X; q.ldx = ldx; q.A = A; q.lda = lda; q.Wb = Wb; q.ldw = ldw; q.bb = bb; q.gt = gt; q.B = B; q.gh = gh; q.gw = gw; q.P = P; q.C = C;
  q.act = act; q.powp = powp; q.inv_count = inv_count; q.accumulate = accumulate != 0; q.dWa = dWa; q.dba = dba; q.dWb = dWb; q.dbb = dbb; q.loss = loss;
  return head_backward_run("head_backward", q, ws, g_op_bf16, (hipStream_t)stream);
}

// ---- tail fit (tailfit.hip) ----
// (the head's condition, inside the widths layernorm_kernel -- and with it the forward's decoder -- takes)
int cs_tail_fit_supported(int hidden, int patch) { return cs_headfit_supported(hidden, patch) && hidden <= 2048; }
int cs_tail_fit_ln_row_tile(void) { return CS_TAILFIT_LN_ROW_TILE; }

size_t cs_ln_backward_workspace_bytes(int M, int C) {
  if (M <= 0 || C < 64 || C % 64 || C > 2048) return 0;
  return cs_ln_backward_workspace(M, C);
}

size_t cs_tail_backward_workspace_bytes(int M, int C, int P) {
  if (M <= 0 || !cs_tail_fit_supported(C, P)) return 0;
  return cs_tail_backward_workspace(M, C);
}

int cs_op_ln_backward(const float* y, int ldy, const float* dx, int ldx, const float* gamma, int M, int C, float eps, int bf16, float inv_count,
                      int accumulate, uint16_t* dyh, int ldd, float* dgamma, float* dbeta, void* ws, cs_stream stream) {
  if (!y || !dx || !gamma || !dyh || !dgamma || !dbeta || !ws) return fail(CS_ERR_BAD_ARG, "ln_backward: null pointer");
  if (M <= 0) return fail(CS_ERR_BAD_ARG, "ln_backward: empty shape");
  if (C < 64 || C % 64 || C > 2048 || M > (1 << 22)) return fail(CS_ERR_UNSUPPORTED, "ln_backward: built for C a multiple of 64 in [64, 2048] and M <= 2^22 (M %d, C %d)", M, C);
  if (ldy < C || ldx < C || ldd < C || ldy % 4 || ldx % 4 || ldd % 4) return fail(CS_ERR_BAD_ARG, "ln_backward: row strides must be multiples of 4 elements and at least C");
  if (!(eps >= 0.f) || !(inv_count > 0.f)) return fail(CS_ERR_BAD_ARG, "ln_backward: eps must be >= 0 and inv_count positive");
  if (bf16 != 0 && bf16 != 1) return fail(CS_ERR_BAD_ARG, "ln_backward: bf16 must be 0 or 1");
  if (misaligned(y, 16) || misaligned(dx, 16) || misaligned(gamma, 16) || misaligned(dyh, 8) || misaligned(dgamma, 4) || misaligned(dbeta, 4) || misaligned(ws, 256))
    return fail(CS_ERR_BAD_ARG, "ln_backward: misaligned pointer (fp32 rows and gamma 16 bytes, dyh 8, the sums 4, workspace 256)");
  CsLnBackward p{};
  p.y = y; p.ldy = ldy; p.dx = dx; p.ldx = ldx; p.gamma = gamma; p.eps = eps; p.M = M; p.C = C; p.scale = inv_count; p.accumulate = accumulate != 0;
  p.dyh = dyh; p.ldd = ldd; p.dgamma = dgamma; p.dbeta = dbeta;
  HIPCHK(cs_ln_backward_launch(&p, ws, bf16, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

// every check of the head's and the tail's backward (cs_op_tail_backward, cs_tail_backward and the cross-attention fit's come through here)
static int tail_backward_check(const char* op, const CsTailBackward& q, void* ws) {
  const CsHeadBackward& hq = q.head;
  if (int r = head_fit_shape_check(op, hq.A, hq.lda, hq.Wb, hq.ldw, hq.bb, hq.gt, hq.B, hq.gh, hq.gw, hq.P, hq.C, hq.act, hq.powp, ws)) return r;
  const int C = hq.C;
  if (!cs_tail_fit_supported(C, hq.P) || (long long)hq.B * hq.gh * hq.gw * C >= (1ll << 31))
    return fail(CS_ERR_UNSUPPORTED, "%s: built for hidden <= 2048 and fewer than 2^31 token elements; split the batch", op);
  if (!hq.X || !hq.dWa || !hq.dba || !hq.dWb || !hq.dbb || !hq.loss || !q.x2 || !q.H || !q.W2 || !q.b2 || !q.gamma3 || !q.Wa || !q.dW1 || !q.db1 ||
      !q.dW2 || !q.db2 || !q.dg3 || !q.db3)
    return fail(CS_ERR_BAD_ARG, "%s: null pointer", op);
  for (int ld : {hq.ldx, q.ldh, q.ldw2, q.ldwa})
    if (ld < C || ld % 8) return fail(CS_ERR_BAD_ARG, "%s: row strides must be multiples of 8 elements and at least C", op);
  if (misaligned(hq.X, 16) || misaligned(q.x2, 16) || misaligned(q.H, 16) || misaligned(q.W2, 16) || misaligned(q.Wa, 16) || misaligned(q.b2, 16) || misaligned(q.gamma3, 16))
    return fail(CS_ERR_BAD_ARG, "%s: misaligned input (16-bit operands, x2, b2 and gamma 16 bytes)", op);
  for (const float* o : {hq.dWa, hq.dba, hq.dWb, hq.dbb, q.dW1, q.db1, q.dW2, q.db2, q.dg3, q.db3})
    if (misaligned(o, 4)) return fail(CS_ERR_BAD_ARG, "%s: misaligned output", op);
  if (misaligned(hq.loss, 8)) return fail(CS_ERR_BAD_ARG, "%s: misaligned output", op);
  if (!(hq.inv_count > 0.0) || !(q.eps >= 0.f)) return fail(CS_ERR_BAD_ARG, "%s: inv_count must be positive and eps >= 0", op);
  return 0;
}

// cs_op_tail_backward and cs_tail_backward come through here: every check of both backwards first, then the launches
int cs_host::tail_backward_run(const char* op, const CsTailBackward& q, void* ws, int bf, hipStream_t st) {
  if (int r = tail_backward_check(op, q, ws)) return r;
  HIPCHK(cs_tail_backward_launch(&q, ws, bf, st));
  return 0;
}

// What the cross-attention block and the self-attention block ask alike of their own operands: the 16-byte inputs `in16`, lse and the fp32
// outputs all there; the row strides `lds`; with kv_rows > 0 the packed K | V rows' stride; the alignments (`x`: the block's fp32 input rows, named
// in the message); and the attention backward's parameters as the launch will queue them.
static int attn_block_check(const char* op, int C, std::initializer_list<const void*> in16, const float* lse, std::initializer_list<const float*> outs,
                            std::initializer_list<int> lds, long long kv_rows, int ldkv, const char* x, const CsAttnBwdParams& a) {
  bool null = !lse, odd = misaligned(lse, 4);
  for (const void* p : in16) { null = null || !p; odd = odd || misaligned(p, 16); }
  for (const float* o : outs) null = null || !o;
  if (null) return fail(CS_ERR_BAD_ARG, "%s: null pointer", op);
  for (int ld : lds)
    if (ld < C || ld % 8) return fail(CS_ERR_BAD_ARG, "%s: row strides must be multiples of 8 elements and at least C", op);
  if (kv_rows > 0 && (ldkv < C || ldkv % 8 || kv_rows * ldkv >= (1ll << 30)))
    return fail(CS_ERR_BAD_ARG, "%s: the K | V row stride must be a multiple of 8 elements, at least C, and N Np times it below 2^30", op);
  if (odd) return fail(CS_ERR_BAD_ARG, "%s: misaligned input (16-bit operands, %s, bo and gamma 16 bytes, lse 4)", op, x);
  for (const float* o : outs)
    if (misaligned(o, 4)) return fail(CS_ERR_BAD_ARG, "%s: misaligned output", op);
  if (const char* e = cs_attnbwd_check(&a)) return fail(CS_ERR_BAD_ARG, "%s: %s", op, e);
  return 0;
}

// every check of the cross-attention fit's backward: the tail's, then the block's own (its attention backward's parameters included)
static int cross_backward_check(const char* op, const CsCrossBackward& q, void* ws, int bf) {
  if (int r = tail_backward_check(op, q.tail, ws)) return r;
  const CsHeadBackward& hq = q.tail.head;
  const int C = hq.C;
  if (q.heads <= 0 || C % q.heads || !cs_attnbwd_supported(C / q.heads))
    return fail(CS_ERR_UNSUPPORTED, "%s: the attention backward is built for head dims 16, 48 and 96 (hidden %d, %d heads)", op, C, q.heads);
  if (q.N <= 0) return fail(CS_ERR_BAD_ARG, "%s: N must be positive", op);
  const long long Mk = (long long)hq.B * hq.gh * hq.gw * q.N;
  if (Mk * 2 * C >= (1ll << 31)) return fail(CS_ERR_UNSUPPORTED, "%s: built for fewer than 2^31 K | V elements; split the batch", op);
  CsAttnBwdParams a{};
  cs_cross_backward_attn_params(&q, ws, bf, &a);
  return attn_block_check(op, C, {q.x1, q.Qp, q.K, q.V, q.O, q.mem, q.W1, q.Wo, q.bo, q.gamma2}, q.lse, {q.dWin, q.dbin, q.dWo, q.dbo, q.dg2, q.db2},
                          {q.ldq, q.ldo, q.ldm, q.ldw1, q.ldwo}, (long long)hq.gh * hq.gw * q.N, q.ldkv, "x1", a);
}

// every check of the whole layer's backward: the cross-attention fit's, then the self-attention block's own
static int layer_backward_check(const char* op, const CsLayerBackward& q, void* ws, int bf) {
  if (int r = cross_backward_check(op, q.cross, ws, bf)) return r;
  const CsHeadBackward& hq = q.cross.tail.head;
  const int C = hq.C;
  if ((long long)hq.B * hq.gh * hq.gw * 3 * C >= (1ll << 31)) return fail(CS_ERR_UNSUPPORTED, "%s: built for fewer than 2^31 Q | K | V elements; split the batch", op);
  CsAttnBwdParams a{};
  cs_layer_backward_attn_params(&q, ws, bf, &a);
  return attn_block_check(op, C, {q.x0, q.Qs, q.Ks, q.Vs, q.Os, q.Wq, q.Wo_s, q.bo_s, q.gamma1}, q.lse_s,
                          {q.dWin_s, q.dbin_s, q.dWo_s, q.dbo_s, q.dg1, q.db1}, {q.ldqkv, q.ldos, q.ldwq, q.ldwos}, 0, 0, "x0", a);
}

// cs_op_cross_backward and cs_cross_backward: every check first, then the launches
int cs_host::cross_backward_run(const char* op, const CsCrossBackward& q, void* ws, int bf, hipStream_t st) {
  if (int r = cross_backward_check(op, q, ws, bf)) return r;
  HIPCHK(cs_cross_backward_launch(&q, ws, bf, st));
  return 0;
}

// cs_op_layer_backward and cs_layer_backward: every check first, then the launches
int cs_host::layer_backward_run(const char* op, const CsLayerBackward& q, void* ws, int bf, hipStream_t st) {
  if (int r = layer_backward_check(op, q, ws, bf)) return r;
  HIPCHK(cs_layer_backward_launch(&q, ws, bf, st));
  return 0;
}

extern "C" {

int cs_op_tail_backward(const float* x2, const uint16_t* H, int ldh, const uint16_t* X, int ldx, const uint16_t* A, int lda, const uint16_t* W2,
                        int ldw2, const float* b2, const float* gamma3, float eps, const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw,
                        const float* bb, const float* gt, int B, int gh, int gw, int P, int C, int act, float powp, double inv_count,
                        int accumulate, float* dW1, float* db1, float* dW2, float* db2, float* dg3, float* db3, float* dWa, float* dba,
                        float* dWb, float* dbb, double* loss, void* ws, cs_stream stream) {
  CsTailBackward q{};
  q.x2 = x2; q.H = H; q.ldh = ldh; q.W2 = W2; q.ldw2 = ldw2; q.b2 = b2; q.gamma3 = gamma3; q.eps = eps; q.Wa = Wa; q.ldwa = ldwa;
  q.dW1 = dW1; q.db1 = db1; q.dW2 = dW2; q.db2 = db2; q.dg3 = dg3; q.db3 = db3;
  CsHeadBackward& hq = q.head;
  hq.X = X; hq.ldx = ldx; hq.A = A; hq.lda = lda; hq.Wb = Wb; hq.ldw = ldw; hq.bb = bb; hq.gt = gt; hq.B = B; hq.gh = gh; hq.gw = gw; hq.P = P; hq.C = C;
  hq.act = act; hq.powp = powp; hq.inv_count = inv_count; hq.accumulate = accumulate != 0; hq.dWa = dWa; hq.dba = dba; hq.dWb = dWb; hq.dbb = dbb;
  hq.loss = loss;
  return tail_backward_run("tail_backward", q, ws, g_op_bf16, (hipStream_t)stream);
}

int cs_op_adamw(float* p, float* m, float* v, const float* g, long long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                int step, uint16_t* p16, cs_stream stream) {
  if (!p || !m || !v || !g) return fail(CS_ERR_BAD_ARG, "adamw: null pointer");
  if (n <= 0 || n > (1ll << 38)) return fail(CS_ERR_BAD_ARG, "adamw: n must be in [1, 2^38]");
  if (step < 1) return fail(CS_ERR_BAD_ARG, "adamw: steps count from 1");
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !(weight_decay >= 0.f))
    return fail(CS_ERR_BAD_ARG, "adamw: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)");
  if (misaligned(p, 4) || misaligned(m, 4) || misaligned(v, 4) || misaligned(g, 4) || misaligned(p16, 2)) return fail(CS_ERR_BAD_ARG, "adamw: misaligned pointer");
  HIPCHK(cs_adamw_launch(p, m, v, g, n, lr, beta1, beta2, eps, weight_decay, step, p16, g_op_bf16, (hipStream_t)stream));
  return 0;
}

// ---- attention backward (attnbwd.hip) ----
size_t cs_attention_backward_workspace_bytes(int batch, int heads, int Lq, int Lk, int dh) {
  if (batch <= 0 || heads <= 0 || Lq <= 0 || Lk <= 0 || !cs_attnbwd_supported(dh)) return 0;
  return cs_attnbwd_workspace(batch, heads, Lq);
}

int cs_attention_backward_tiles(int dh, int* q_tile, int* k_tile) {
  if (!cs_attnbwd_supported(dh)) return fail(CS_ERR_UNSUPPORTED, "attention_backward: built for head dims 16, 48 and 96 (got %d)", dh);
  if (q_tile) *q_tile = 64;
  if (k_tile) *k_tile = 64;
  return 0;
}

int cs_op_attention_backward(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* O, const uint16_t* dO, const float* lse,
                             int ldq, int ldk, int ldv, int ldo, int lddo, long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                             long long do_bs, int batch, int heads, int Lq, int Lk, int dh, float q_scale, uint16_t* dQ, int lddq,
                             long long dq_bs, uint16_t* dK, int lddk, long long dk_bs, uint16_t* dV, int lddv, long long dv_bs, void* ws,
                             cs_stream stream) {
  CsAttnBwdParams a{};
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.dO = dO; a.lse = lse; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo;
  a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs; a.do_bs = do_bs; a.nbatch = batch; a.heads = heads; a.Lq = Lq; a.Lk = Lk;
  a.dQ = dQ; a.lddq = lddq; a.dq_bs = dq_bs; a.dK = dK; a.lddk = lddk; a.dk_bs = dk_bs; a.dV = dV; a.lddv = lddv; a.dv_bs = dv_bs;
  a.D = static_cast<float*>(ws); a.bf16 = g_op_bf16;
  if (!(q_scale >= 0.f)) return fail(CS_ERR_BAD_ARG, "attention_backward: q_scale must be >= 0 (0 = log2(e)/sqrt(dh))");
  if (const char* e = cs_attnbwd_check(&a)) return fail(CS_ERR_BAD_ARG, "%s", e);
  if (!cs_attnbwd_supported(dh)) return fail(CS_ERR_UNSUPPORTED, "attention_backward: built for head dims 16, 48 and 96 (got %d)", dh);
  a.scale_log2e = q_scale == 0.f ? LOG2E / std::sqrt((float)dh) : q_scale;
  HIPCHK(cs_attnbwd_launch(&a, dh, (hipStream_t)stream));
  return 0;
}

// ---- cross-attention fit (crossfit.hip) ----
int cs_cross_fit_supported(int hidden, int heads, int patch) {
  return cs_tail_fit_supported(hidden, patch) && heads > 0 && hidden % heads == 0 && cs_attnbwd_supported(hidden / heads);
}

size_t cs_cross_backward_workspace_bytes(int B, int Np, int N, int C, int P, int heads) {
  if (B <= 0 || Np <= 0 || N <= 0 || !cs_cross_fit_supported(C, heads, P) || (long long)B * Np * N * 2 * C >= (1ll << 31)) return 0;
  return cs_cross_backward_workspace(B, Np, N, C, heads);
}

int cs_op_cross_backward(const float* x1, const uint16_t* Qp, int ldq, const uint16_t* K, const uint16_t* V, int ldkv, const uint16_t* O, int ldo,
                         const float* lse, const uint16_t* mem, int ldm, const uint16_t* W1, int ldw1, const uint16_t* Wo, int ldwo, const float* bo,
                         const float* gamma2, int N, int heads, int short_cut, const float* x2, const uint16_t* H, int ldh, const uint16_t* X,
                         int ldx, const uint16_t* A, int lda, const uint16_t* W2, int ldw2, const float* b2, const float* gamma3, float eps,
                         const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                         int C, int act, float powp, double inv_count, int accumulate, float* dWin, float* dbin, float* dWo, float* dbo,
                         float* dgamma2, float* dbeta2, float* dW1, float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa,
                         float* dba, float* dWb, float* dbb, double* loss, void* ws, cs_stream stream) {
  CsCrossBackward c{};
  c.x1 = x1; c.Qp = Qp; c.ldq = ldq; c.K = K; c.V = V; c.ldkv = ldkv; c.O = O; c.ldo = ldo; c.lse = lse; c.mem = mem; c.ldm = ldm;
  c.W1 = W1; c.ldw1 = ldw1; c.Wo = Wo; c.ldwo = ldwo; c.bo = bo; c.gamma2 = gamma2; c.N = N; c.heads = heads; c.short_cut = short_cut != 0;
  c.dWin = dWin; c.dbin = dbin; c.dWo = dWo; c.dbo = dbo; c.dg2 = dgamma2; c.db2 = dbeta2;
  CsTailBackward& q = c.tail;
  q.x2 = x2; q.H = H; q.ldh = ldh; q.W2 = W2; q.ldw2 = ldw2; q.b2 = b2; q.gamma3 = gamma3; q.eps = eps; q.Wa = Wa; q.ldwa = ldwa;
  q.dW1 = dW1; q.db1 = db1; q.dW2 = dW2; q.db2 = db2; q.dg3 = dgamma3; q.db3 = dbeta3;
  CsHeadBackward& hq = q.head;
  hq.X = X; hq.ldx = ldx; hq.A = A; hq.lda = lda; hq.Wb = Wb; hq.ldw = ldw; hq.bb = bb; hq.gt = gt; hq.B = B; hq.gh = gh; hq.gw = gw; hq.P = P; hq.C = C;
  hq.act = act; hq.powp = powp; hq.inv_count = inv_count; hq.accumulate = accumulate != 0; hq.dWa = dWa; hq.dba = dba; hq.dWb = dWb; hq.dbb = dbb;
  hq.loss = loss;
  return cross_backward_run("cross_backward", c, ws, g_op_bf16, (hipStream_t)stream);
}

// ---- whole-layer fit (layerfit.hip) ----
int cs_layer_fit_supported(int hidden, int heads, int patch, int do_self_attn) { return do_self_attn != 0 && cs_cross_fit_supported(hidden, heads, patch); }

size_t cs_layer_backward_workspace_bytes(int B, int Np, int N, int C, int P, int heads) {
  if (!cs_cross_backward_workspace_bytes(B, Np, N, C, P, heads) || (long long)B * Np * 3 * C >= (1ll << 31)) return 0;
  return cs_layer_backward_workspace(B, Np, N, C, heads);
}

int cs_op_layer_backward(const float* x0, const uint16_t* Qs, const uint16_t* Ks, const uint16_t* Vs, int ldqkv, const uint16_t* Os, int ldos,
                         const float* lse_s, const uint16_t* Wq, int ldwq, const uint16_t* Wo_s, int ldwos, const float* bo_s, const float* gamma1,
                         const float* x1, const uint16_t* Qp, int ldq, const uint16_t* K, const uint16_t* V, int ldkv, const uint16_t* O, int ldo,
                         const float* lse, const uint16_t* mem, int ldm, const uint16_t* W1, int ldw1, const uint16_t* Wo, int ldwo, const float* bo,
                         const float* gamma2, int N, int heads, int short_cut, const float* x2, const uint16_t* H, int ldh, const uint16_t* X,
                         int ldx, const uint16_t* A, int lda, const uint16_t* W2, int ldw2, const float* b2, const float* gamma3, float eps,
                         const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                         int C, int act, float powp, double inv_count, int accumulate, float* dWin_s, float* dbin_s, float* dWo_s, float* dbo_s,
                         float* dgamma1, float* dbeta1, float* dWin, float* dbin, float* dWo, float* dbo, float* dgamma2, float* dbeta2, float* dW1,
                         float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa, float* dba, float* dWb, float* dbb,
                         double* loss, void* ws, cs_stream stream) {
  CsLayerBackward y{};
  y.x0 = x0; y.Qs = Qs; y.Ks = Ks; y.Vs = Vs; y.ldqkv = ldqkv; y.Os = Os; y.ldos = ldos; y.lse_s = lse_s; y.Wq = Wq; y.ldwq = ldwq;
  y.Wo_s = Wo_s; y.ldwos = ldwos; y.bo_s = bo_s; y.gamma1 = gamma1;
  y.dWin_s = dWin_s; y.dbin_s = dbin_s; y.dWo_s = dWo_s; y.dbo_s = dbo_s; y.dg1 = dgamma1; y.db1 = dbeta1;
  CsCrossBackward& c = y.cross;
  c.x1 = x1; c.Qp = Qp; c.ldq = ldq; c.K = K; c.V = V; c.ldkv = ldkv; c.O = O; c.ldo = ldo; c.lse = lse; c.mem = mem; c.ldm = ldm;
  c.W1 = W1; c.ldw1 = ldw1; c.Wo = Wo; c.ldwo = ldwo; c.bo = bo; c.gamma2 = gamma2; c.N = N; c.heads = heads; c.short_cut = short_cut != 0;
  c.dWin = dWin; c.dbin = dbin; c.dWo = dWo; c.dbo = dbo; c.dg2 = dgamma2; c.db2 = dbeta2;
  CsTailBackward& q = c.tail;
  q.x2 = x2; q.H = H; q.ldh = ldh; q.W2 = W2; q.ldw2 = ldw2; q.b2 = b2; q.gamma3 = gamma3; q.eps = eps; q.Wa = Wa; q.ldwa = ldwa;
  q.dW1 = dW1; q.db1 = db1; q.dW2 = dW2; q.db2 = db2; q.dg3 = dgamma3; q.db3 = dbeta3;
  CsHeadBackward& hq = q.head;
  hq.X = X; hq.ldx = ldx; hq.A = A; hq.lda = lda; hq.Wb = Wb; hq.ldw = ldw; hq.bb = bb; hq.gt = gt; hq.B = B; hq.gh = gh; hq.gw = gw; hq.P = P; hq.C = C;
  hq.act = act; hq.powp = powp; hq.inv_count = inv_count; hq.accumulate = accumulate != 0; hq.dWa = dWa; hq.dba = dba; hq.dWb = dWb; hq.dbb = dbb;
  hq.loss = loss;
  return layer_backward_run("layer_backward", y, ws, g_op_bf16, (hipStream_t)stream);
}

}  // extern "C"

// ---- the backwards on a handle: the backward of a fit scope over what the last forward left behind ----
// The scopes are nested.  FIT_HEAD (f15) is the regression head; the closing launch of the decoder writes the normalised rows in fp32 (p.xq) and,
// where the head's first linear rides along (rowln.hip), no 16-bit copy, so X is rounded here from p.xq, the rounding the forward's own operand
// went through.  FIT_TAIL (f16) adds the last layer's feed-forward block and norm3: the last forward must have kept x2 and H (cs_fit_tail_keep).
// FIT_CROSS (f17) adds that layer's cross-attention and norm2: x1 and lse kept as well (cs_fit_cross_keep).  FIT_LAYER (f18) adds its self-attention
// and norm1: x0, Os and the self-attention's lse kept as well (cs_fit_layer_keep).  The workspace of a backward is the handle's own allocation
// (X, then the scope's cs_*_backward_workspace, each of which begins with its parent's), grown like the forward's.
namespace {

int last_rows(const cs_model* h) { return h->last_fwd.B * (h->last_fwd.H / h->cfg.patch) * (h->last_fwd.W / h->cfg.patch); }

// the handle's ONE kept region as the last forward carved it: at the level it kept for
cs_fit::Kept last_kept(const cs_model* h) {
  const cs_model::LastForward& lf = h->last_fwd;
  return cs_fit::kept_carve(h->fit_kept, lf.kept, lf.B, last_rows(h) / lf.B, h->cfg.hidden, h->cfg.dec_heads);
}

// the workspace of one backward of `scope` (each begins with its parent's)
size_t backward_workspace(FitScope scope, int B, int Np, int N, int C, int heads) {
  if (scope == FIT_LAYER) return cs_layer_backward_workspace(B, Np, N, C, heads);
  if (scope == FIT_CROSS) return cs_cross_backward_workspace(B, Np, N, C, heads);
  return scope == FIT_TAIL ? cs_tail_backward_workspace(B * Np, C) : cs_head_backward_workspace(B * Np, C);
}

// what a caller of the backwards can get wrong, refused before fit_inputs allocates or queues the rounding of X (the *_backward_run check again)
int fit_args_check(const char* op, const cs_model* h, int B, const float* gt, std::initializer_list<const float*> outs, const double* loss,
                   double inv_count, bool needs_decoder) {
  if (B <= 0) return fail(CS_ERR_BAD_ARG, "%s: empty batch", op);
  bool null = !gt || !loss;
  uintptr_t bits = (uintptr_t)gt;
  for (const float* o : outs) { null = null || !o; bits |= (uintptr_t)o; }
  if (null) return fail(CS_ERR_BAD_ARG, "%s: null pointer", op);
  if ((bits & 3) || ((uintptr_t)loss & 7)) return fail(CS_ERR_BAD_ARG, "%s: misaligned pointer (fp32 4 bytes, the loss 8)", op);
  if (!(inv_count > 0.0)) return fail(CS_ERR_BAD_ARG, "%s: inv_count must be positive", op);
  if (h && h->cfg.act == 1 && h->cfg.pow_p != 1.0f) return fail(CS_ERR_UNSUPPORTED, "%s: tanh with a power factor other than 1 is not built", op);
  if (needs_decoder && h && h->finalized && h->dec.empty()) return fail(CS_ERR_STATE, "%s: the handle has no decoder layer", op);
  return 0;
}

// the state a fit call of `scope` needs, without touching the handle; B > 0: the shape the caller names is the last forward's
int fit_state_check(cs_model* h, int B, int H, int W, const char* op, FitScope scope) {
  if (!h) return fail(CS_ERR_BAD_ARG, "null handle");
  if (!h->finalized) return fail(CS_ERR_STATE, "%s before cs_finalize", op);
  const cs_model::LastForward& lf = h->last_fwd;
  if (!lf.ok || lf.mode < 0) return fail(CS_ERR_STATE, "%s: no successful cs_forward* call on this handle yet", op);
  if (lf.mode == 2) return fail(CS_ERR_STATE, "%s: the last call on this handle only encoded references", op);
  if (B > 0 && (lf.B != B || lf.H != H || lf.W != W))
    return fail(CS_ERR_STATE, "%s: the last forward ran (B %d, H %d, W %d), this call names (%d, %d, %d)", op, lf.B, lf.H, lf.W, B, H, W);
  const cs_config& c = h->cfg;
  if (!cs_headfit_supported(c.hidden, c.patch)) return fail(CS_ERR_UNSUPPORTED, "%s: built for hidden a multiple of 64 and patch 14 (hidden %d, patch %d)", op, c.hidden, c.patch);
  if (scope >= FIT_TAIL && !cs_tail_fit_supported(c.hidden, c.patch)) return fail(CS_ERR_UNSUPPORTED, "%s: built for hidden <= 2048 (hidden %d)", op, c.hidden);
  if (scope >= FIT_CROSS && !cs_cross_fit_supported(c.hidden, c.dec_heads, c.patch))
    return fail(CS_ERR_UNSUPPORTED, "%s: the attention backward is built for head dims 16, 48 and 96 (hidden %d, %d heads)", op, c.hidden, c.dec_heads);
  if (scope >= FIT_LAYER && !c.do_self_attn) return fail(CS_ERR_UNSUPPORTED, "%s: the decoder has no self-attention (decoder_do_self_attn = 0): nothing to fit", op);
  if (scope >= FIT_LAYER && lf.kept < FIT_LAYER) return fail(CS_ERR_STATE, "%s: the last forward on this handle ran with cs_fit_layer_keep off", op);
  if (scope >= FIT_CROSS && lf.kept < FIT_CROSS) return fail(CS_ERR_STATE, "%s: the last forward on this handle ran with cs_fit_cross_keep off", op);
  if (scope >= FIT_TAIL && lf.kept < FIT_TAIL) return fail(CS_ERR_STATE, "%s: the last forward on this handle ran with cs_fit_tail_keep off", op);
  return 0;
}

// the three cs_debug_*_inputs: the caller's row count against the last forward's, where there is one (fit_state_check refuses the rest)
int debug_rows_check(const cs_model* h, int rows, const char* op) {
  if (h && h->finalized && h->last_fwd.ok && h->last_fwd.mode != 2 && rows != last_rows(h))
    return fail(CS_ERR_BAD_ARG, "%s: the last forward left %d rows, the caller names %d", op, last_rows(h), rows);
  return 0;
}

// What a backward of `scope` starts from: the last forward's rows M, X (M, C) rounded to 16 bits at the front of the handle's region, and the
// scope's workspace behind it.  Enters the call (call_enter): the caller leaves it with call_leave.
struct FitIn { int M = 0; h16_t* X = nullptr; void* ws = nullptr; };
int fit_inputs(cs_model* h, int B, int H, int W, hipStream_t st, const char* op, FitScope scope, FitIn* in) {
  if (int r = fit_state_check(h, B, H, W, op, scope)) return r;
  const cs_model::LastForward& lf = h->last_fwd;
  const cs_config& c = h->cfg;
  const int M = last_rows(h), C = c.hidden;
  const size_t xbytes = cs_fit::up256((size_t)M * C * 2), need = xbytes + backward_workspace(scope, lf.B, M / lf.B, lf.N, C, c.dec_heads);
  if (int r = call_enter(h, st)) return r;
  if (int r = grow_retired(h, &h->hfit_ws, &h->hfit_ws_bytes, need, st)) return r;
  in->M = M; in->X = static_cast<h16_t*>(h->hfit_ws); in->ws = static_cast<char*>(h->hfit_ws) + xbytes;
  HIPCHK(cs_pack_f16_launch(lf.xq, M, C, in->X, C, nullptr, nullptr, c.operand_dtype, st));
  return 0;
}

// the end of a backward on a handle: the call is left whatever the run returned
int fit_leave(cs_model* h, hipStream_t st, int rc) {
  const int r = call_leave(h, st);
  return r ? r : rc;
}

CsHeadBackward fill_head_backward(const cs_model* h, const h16_t* X, const float* gt, int B, int H, int W, double inv_count, int accumulate,
                                  float* dWa, float* dba, float* dWb, float* dbb, double* loss) {
  const cs_config& c = h->cfg;
  const int C = c.hidden;
  CsHeadBackward q{};
  q.X = X; q.ldx = C; q.A = h->last_fwd.dhid; q.lda = C; q.Wb = h->Wh2; q.ldw = C; q.bb = h->bh2; q.gt = gt; q.B = B; q.gh = H / c.patch; q.gw = W / c.patch;
  q.P = c.patch; q.C = C; q.act = c.act; q.powp = c.pow_p; q.inv_count = inv_count; q.accumulate = accumulate != 0;
  q.dWa = dWa; q.dba = dba; q.dWb = dWb; q.dbb = dbb; q.loss = loss;
  return q;
}

// (everything but .head)
CsTailBackward fill_tail_backward(const cs_model* h, float* dW1, float* db1, float* dW2, float* db2, float* dg3, float* db3) {
  const int C = h->cfg.hidden;
  const DecLayer& D = h->dec.back();
  const cs_fit::Kept k = last_kept(h);
  CsTailBackward q{};
  q.x2 = k.x2; q.H = k.H; q.ldh = C;
  q.W2 = D.l2W; q.ldw2 = C; q.b2 = D.l2b; q.gamma3 = D.n3g; q.eps = 1e-5f; q.Wa = h->Wh0; q.ldwa = C;
  q.dW1 = dW1; q.db1 = db1; q.dW2 = dW2; q.db2 = db2; q.dg3 = dg3; q.db3 = db3;
  return q;
}

// (everything but .tail)
CsCrossBackward fill_cross_backward(const cs_model* h, float* dWin, float* dbin, float* dWo, float* dbo, float* dgamma2, float* dbeta2) {
  const cs_config& c = h->cfg;
  const int C = c.hidden;
  const DecLayer& D = h->dec.back();
  const cs_model::LastForward& lf = h->last_fwd;
  CsCrossBackward x{};
  x.x1 = last_kept(h).x1; x.Qp = lf.dq; x.ldq = C; x.K = lf.k; x.V = lf.k + C; x.ldkv = lf.ldkv; x.O = lf.dob; x.ldo = C;
  x.lse = lf.lse; x.mem = lf.mem; x.ldm = C; x.W1 = D.l1W; x.ldw1 = C; x.Wo = D.ca_Wo; x.ldwo = C; x.bo = D.ca_bo; x.gamma2 = D.n2g;
  x.N = lf.N; x.heads = c.dec_heads; x.short_cut = c.do_short_cut != 0;
  x.dWin = dWin; x.dbin = dbin; x.dWo = dWo; x.dbo = dbo; x.dg2 = dgamma2; x.db2 = dbeta2;
  return x;
}

// (everything but .cross)
CsLayerBackward fill_layer_backward(const cs_model* h, float* dWin_s, float* dbin_s, float* dWo_s, float* dbo_s, float* dgamma1, float* dbeta1) {
  const int C = h->cfg.hidden;
  const DecLayer& D = h->dec.back();
  const cs_model::LastForward& lf = h->last_fwd;
  const cs_fit::Kept k = last_kept(h);
  CsLayerBackward y{};
  y.x0 = k.x0; y.Qs = lf.dqkv; y.Ks = lf.dqkv + C; y.Vs = lf.dqkv + 2 * C; y.ldqkv = 3 * C; y.Os = k.Os; y.ldos = C;
  y.lse_s = k.lse_s; y.Wq = D.ca_Wq; y.ldwq = C; y.Wo_s = D.sa_Wo; y.ldwos = C; y.bo_s = D.sa_bo; y.gamma1 = D.n1g;
  y.dWin_s = dWin_s; y.dbin_s = dbin_s; y.dWo_s = dWo_s; y.dbo_s = dbo_s; y.dg1 = dgamma1; y.db1 = dbeta1;
  return y;
}

}  // namespace

extern "C" {

int cs_head_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWa, float* dba, float* dWb,
                     float* dbb, double* loss, cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = fit_args_check("cs_head_backward", h, B, gt, {dWa, dba, dWb, dbb}, loss, inv_count, false)) return r;
  FitIn in;
  if (int r = fit_inputs(h, B, H, W, st, "cs_head_backward", FIT_HEAD, &in)) return r;
  const CsHeadBackward q = fill_head_backward(h, in.X, gt, B, H, W, inv_count, accumulate, dWa, dba, dWb, dbb, loss);
  return fit_leave(h, st, head_backward_run("cs_head_backward", q, in.ws, h->cfg.operand_dtype, st));
}

int cs_debug_head_inputs(cs_handle h, uint16_t* X_out, uint16_t* A_out, int rows, cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = debug_rows_check(h, rows, "cs_debug_head_inputs")) return r;
  FitIn in;
  if (int r = fit_inputs(h, 0, 0, 0, st, "cs_debug_head_inputs", FIT_HEAD, &in)) return r;
  const size_t bytes = (size_t)in.M * h->cfg.hidden * 2;
  if (X_out) HIPCHK(hipMemcpyAsync(X_out, in.X, bytes, hipMemcpyDeviceToDevice, st));
  if (A_out) HIPCHK(hipMemcpyAsync(A_out, h->last_fwd.dhid, bytes, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

int cs_tail_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dW1, float* db1, float* dW2,
                     float* db2, float* dg3, float* db3, float* dWa, float* dba, float* dWb, float* dbb, double* loss, cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = fit_args_check("cs_tail_backward", h, B, gt, {dW1, db1, dW2, db2, dg3, db3, dWa, dba, dWb, dbb}, loss, inv_count, true)) return r;
  FitIn in;
  if (int r = fit_inputs(h, B, H, W, st, "cs_tail_backward", FIT_TAIL, &in)) return r;
  CsTailBackward q = fill_tail_backward(h, dW1, db1, dW2, db2, dg3, db3);
  q.head = fill_head_backward(h, in.X, gt, B, H, W, inv_count, accumulate, dWa, dba, dWb, dbb, loss);
  return fit_leave(h, st, tail_backward_run("cs_tail_backward", q, in.ws, h->cfg.operand_dtype, st));
}

int cs_debug_tail_inputs(cs_handle h, float* x2_out, uint16_t* H_out, int rows, cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = debug_rows_check(h, rows, "cs_debug_tail_inputs")) return r;
  FitIn in;
  if (int r = fit_inputs(h, 0, 0, 0, st, "cs_debug_tail_inputs", FIT_TAIL, &in)) return r;
  const size_t n = (size_t)in.M * h->cfg.hidden;
  const cs_fit::Kept k = last_kept(h);
  if (x2_out) HIPCHK(hipMemcpyAsync(x2_out, k.x2, n * 4, hipMemcpyDeviceToDevice, st));
  if (H_out) HIPCHK(hipMemcpyAsync(H_out, k.H, n * 2, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

int cs_cross_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWin, float* dbin, float* dWo,
                      float* dbo, float* dgamma2, float* dbeta2, float* dW1, float* db1, float* dW2, float* db2, float* dg3, float* db3, float* dWa,
                      float* dba, float* dWb, float* dbb, double* loss, cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = fit_args_check("cs_cross_backward", h, B, gt, {dWin, dbin, dWo, dbo, dgamma2, dbeta2, dW1, db1, dW2, db2, dg3, db3, dWa, dba, dWb, dbb},
                             loss, inv_count, true))
    return r;
  FitIn in;
  if (int r = fit_inputs(h, B, H, W, st, "cs_cross_backward", FIT_CROSS, &in)) return r;
  CsCrossBackward x = fill_cross_backward(h, dWin, dbin, dWo, dbo, dgamma2, dbeta2);
  x.tail = fill_tail_backward(h, dW1, db1, dW2, db2, dg3, db3);
  x.tail.head = fill_head_backward(h, in.X, gt, B, H, W, inv_count, accumulate, dWa, dba, dWb, dbb, loss);
  return fit_leave(h, st, cross_backward_run("cs_cross_backward", x, in.ws, h->cfg.operand_dtype, st));
}

int cs_debug_cross_inputs(cs_handle h, float* x1_out, uint16_t* q_out, uint16_t* o_out, float* lse_out, uint16_t* k_out, uint16_t* v_out, int rows,
                          cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = debug_rows_check(h, rows, "cs_debug_cross_inputs")) return r;
  // (the state checks alone: six copies need neither X nor the backward's workspace, which fit_inputs would grow the handle's region to)
  if (int r = fit_state_check(h, 0, 0, 0, "cs_debug_cross_inputs", FIT_CROSS)) return r;
  if (int r = call_enter(h, st)) return r;
  const cs_model::LastForward& lf = h->last_fwd;
  const size_t M = last_rows(h), C = h->cfg.hidden, n = M * C, Mk = M * lf.N;
  if (x1_out) HIPCHK(hipMemcpyAsync(x1_out, last_kept(h).x1, n * 4, hipMemcpyDeviceToDevice, st));
  if (q_out) HIPCHK(hipMemcpyAsync(q_out, lf.dq, n * 2, hipMemcpyDeviceToDevice, st));
  if (o_out) HIPCHK(hipMemcpyAsync(o_out, lf.dob, n * 2, hipMemcpyDeviceToDevice, st));
  if (lse_out) HIPCHK(hipMemcpyAsync(lse_out, lf.lse, M * h->cfg.dec_heads * 4, hipMemcpyDeviceToDevice, st));
  if (k_out) HIPCHK(hipMemcpy2DAsync(k_out, C * 2, lf.k, (size_t)lf.ldkv * 2, C * 2, Mk, hipMemcpyDeviceToDevice, st));
  if (v_out) HIPCHK(hipMemcpy2DAsync(v_out, C * 2, lf.k + C, (size_t)lf.ldkv * 2, C * 2, Mk, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

int cs_layer_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWin_s, float* dbin_s, float* dWo_s,
                      float* dbo_s, float* dgamma1, float* dbeta1, float* dWin, float* dbin, float* dWo, float* dbo, float* dgamma2, float* dbeta2,
                      float* dW1, float* db1, float* dW2, float* db2, float* dg3, float* db3, float* dWa, float* dba, float* dWb, float* dbb, double* loss,
                      cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = fit_args_check("cs_layer_backward", h, B, gt, {dWin_s, dbin_s, dWo_s, dbo_s, dgamma1, dbeta1, dWin, dbin, dWo, dbo, dgamma2, dbeta2, dW1, db1,
                                                             dW2, db2, dg3, db3, dWa, dba, dWb, dbb},
                             loss, inv_count, true))
    return r;
  FitIn in;
  if (int r = fit_inputs(h, B, H, W, st, "cs_layer_backward", FIT_LAYER, &in)) return r;
  CsLayerBackward y = fill_layer_backward(h, dWin_s, dbin_s, dWo_s, dbo_s, dgamma1, dbeta1);
  y.cross = fill_cross_backward(h, dWin, dbin, dWo, dbo, dgamma2, dbeta2);
  y.cross.tail = fill_tail_backward(h, dW1, db1, dW2, db2, dg3, db3);
  y.cross.tail.head = fill_head_backward(h, in.X, gt, B, H, W, inv_count, accumulate, dWa, dba, dWb, dbb, loss);
  return fit_leave(h, st, layer_backward_run("cs_layer_backward", y, in.ws, h->cfg.operand_dtype, st));
}

int cs_debug_layer_inputs(cs_handle h, float* x0_out, uint16_t* q_out, uint16_t* k_out, uint16_t* v_out, uint16_t* o_out, float* lse_out, int rows,
                          cs_stream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int r = debug_rows_check(h, rows, "cs_debug_layer_inputs")) return r;
  if (int r = fit_state_check(h, 0, 0, 0, "cs_debug_layer_inputs", FIT_LAYER)) return r;  // (the state checks alone, as cs_debug_cross_inputs)
  if (int r = call_enter(h, st)) return r;
  const cs_model::LastForward& lf = h->last_fwd;
  const size_t M = last_rows(h), C = h->cfg.hidden, n = M * C;
  const cs_fit::Kept k = last_kept(h);
  if (x0_out) HIPCHK(hipMemcpyAsync(x0_out, k.x0, n * 4, hipMemcpyDeviceToDevice, st));
  uint16_t* const outs[3] = {q_out, k_out, v_out};
  for (int j = 0; j < 3; ++j)
    if (outs[j]) HIPCHK(hipMemcpy2DAsync(outs[j], C * 2, lf.dqkv + j * C, 3 * C * 2, C * 2, M, hipMemcpyDeviceToDevice, st));
  if (o_out) HIPCHK(hipMemcpyAsync(o_out, k.Os, n * 2, hipMemcpyDeviceToDevice, st));
  if (lse_out) HIPCHK(hipMemcpyAsync(lse_out, k.lse_s, M * h->cfg.dec_heads * 4, hipMemcpyDeviceToDevice, st));
  return call_leave(h, st);
}

}  // extern "C"
