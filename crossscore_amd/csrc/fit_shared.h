// What headfit.hip, tailfit.hip, crossfit.hip, layerfit.hip and the host files share: the scope enum, the 256-byte rounding, ONE
// carve per backward workspace and one for what a forward keeps, and the block steps every scope's launch is made of (through a weight, the
// backward of a post-norm closing, the backward of an attention block).  The scopes are nested -- the tail's workspace begins with the head's,
// the cross-attention fit's with the tail's, the whole layer's with the cross-attention fit's -- and so are the carves: a launch reads its
// parent's pieces (dpre; dyh and dH; dy2h and dQu) from the parent's carve.  `end` is the workspace's size in bytes, so the size a caller
// allocates by is the carve over a null base that the launch takes its pointers from.
#pragma once
#include "cs_common.h"

#include <cmath>

// The fit scopes, each with its parent in front of it.  Also the level of what a forward kept for the backwards: FIT_HEAD = nothing beyond its own
// workspace, FIT_TAIL = x2 and H, FIT_CROSS = x1 as well, FIT_LAYER = x0, Os and the self-attention's lse as well (kept_carve below).
enum FitScope { FIT_HEAD, FIT_TAIL, FIT_CROSS, FIT_LAYER };

namespace cs_fit {

inline size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// hands out the pieces of a workspace in order, each rounded up to 256 bytes
struct Carver {
  uintptr_t base, at;
  Carver(void* b, size_t skip = 0) : base(reinterpret_cast<uintptr_t>(b)), at(base + skip) {}
  template <class T> T* take(size_t bytes) { T* p = reinterpret_cast<T*>(at); at += up256(bytes); return p; }
  size_t end() const { return at - base; }
};

// the head's backward: g (M, 224), dpre (M, C), WbT (C, 224), the loss partials, gemm_tn's partials
struct HeadWs { h16_t *g, *dpre, *WbT; void *zws, *tws; size_t end; };
inline HeadWs head_carve(void* base, int M, int C) {
  Carver w(base);
  HeadWs k{};
  k.g = w.take<h16_t>((size_t)M * CS_HEADFIT_NPAD * 2);
  k.dpre = w.take<h16_t>((size_t)M * C * 2);
  k.WbT = w.take<h16_t>((size_t)C * CS_HEADFIT_NPAD * 2);
  k.zws = w.take<char>(cs_head_grad_z_workspace(M));
  k.tws = w.take<char>(cs_gemm_tn_workspace(M, C > CS_HEADFIT_NPAD ? C : CS_HEADFIT_NPAD, C));
  k.end = w.end();
  return k;
}

// the tail's: the head's, the transposed weight (C, C), a zero bias (C), dX and y (M, C) fp32, dyh, dH and x2h (M, C) 16 bit, ln_backward's
// partials, gemm_tn's partials
struct TailWs { HeadWs head; h16_t* WT; float *zb, *dX, *y; h16_t *dyh, *dH, *x2h; void *lws, *tws; size_t end; };
inline TailWs tail_carve(void* base, int M, int C) {
  const size_t mc = (size_t)M * C;
  TailWs k{};
  k.head = head_carve(base, M, C);
  Carver w(base, k.head.end);
  k.WT = w.take<h16_t>((size_t)C * C * 2);
  k.zb = w.take<float>((size_t)C * 4);
  k.dX = w.take<float>(mc * 4);
  k.y = w.take<float>(mc * 4);
  k.dyh = w.take<h16_t>(mc * 2);
  k.dH = w.take<h16_t>(mc * 2);
  k.x2h = w.take<h16_t>(mc * 2);
  k.lws = w.take<char>(cs_ln_backward_workspace(M, C));
  k.tws = w.take<char>(cs_gemm_tn_workspace(M, C, C));
  k.end = w.end();
  return k;
}

// The cross-attention fit's: the tail's (tail_carve, which leaves dyh and dHh there), the transposed weight (C, C), a zero bias (C), f32(dyh), dx2
// and y2 (M, C) fp32, dy2h, dOh, x1h and dQu (M, C) 16 bit, dKu | dV (Mk, 2C) 16 bit, the attention backward's, ln_backward's partials, gemm_tn's
// partials for the longer of the two row counts
struct CrossWs {
  const h16_t *dyh, *dHh; h16_t* WT; float *zb, *dyf, *dx2, *y2; h16_t *dy2h, *dOh, *x1h, *dQu, *dKV; void *aws, *lws, *tws; size_t end;
};
inline CrossWs cross_carve(void* base, int B, int Np, int N, int C, int heads) {
  const int M = B * Np, Mk = M * N;
  const size_t mc = (size_t)M * C;
  const TailWs t = tail_carve(base, M, C);
  Carver w(base, t.end);
  CrossWs k{};
  k.dyh = t.dyh; k.dHh = t.dH;
  k.WT = w.take<h16_t>((size_t)C * C * 2);
  k.zb = w.take<float>((size_t)C * 4);
  k.dyf = w.take<float>(mc * 4);
  k.dx2 = w.take<float>(mc * 4);
  k.y2 = w.take<float>(mc * 4);
  k.dy2h = w.take<h16_t>(mc * 2);
  k.dOh = w.take<h16_t>(mc * 2);
  k.x1h = w.take<h16_t>(mc * 2);
  k.dQu = w.take<h16_t>(mc * 2);
  k.dKV = w.take<h16_t>((size_t)Mk * 2 * C * 2);
  k.aws = w.take<char>(cs_attnbwd_workspace(B, heads, Np));
  k.lws = w.take<char>(cs_ln_backward_workspace(M, C));
  k.tws = w.take<char>(cs_gemm_tn_workspace(Mk > M ? Mk : M, C, C));
  k.end = w.end();
  return k;
}

// The whole layer's: the cross-attention fit's (cross_carve, which leaves dy2h and dQu there), the transposed weight (C, C), a zero bias (C),
// dx1 and y1 (M, C) fp32, dy1h, dOsh and x0h (M, C) 16 bit, dQu_s | dKu_s | dV_s (M, 3C) 16 bit, the
// attention backward's, ln_backward's partials, gemm_tn's partials
struct LayerWs {
  const h16_t *dy2h, *dQu; h16_t* WT; float *zb, *dx1, *y1; h16_t *dy1h, *dOsh, *x0h, *dQKV; void *aws, *lws, *tws; size_t end;
};
inline LayerWs layer_carve(void* base, int B, int Np, int N, int C, int heads) {
  const int M = B * Np;
  const size_t mc = (size_t)M * C;
  const CrossWs x = cross_carve(base, B, Np, N, C, heads);
  Carver w(base, x.end);
  LayerWs k{};
  k.dy2h = x.dy2h; k.dQu = x.dQu;
  k.WT = w.take<h16_t>((size_t)C * C * 2);
  k.zb = w.take<float>((size_t)C * 4);
  k.dx1 = w.take<float>(mc * 4);
  k.y1 = w.take<float>(mc * 4);
  k.dy1h = w.take<h16_t>(mc * 2);
  k.dOsh = w.take<h16_t>(mc * 2);
  k.x0h = w.take<h16_t>(mc * 2);
  k.dQKV = w.take<h16_t>(mc * 3 * 2);
  k.aws = w.take<char>(cs_attnbwd_workspace(B, heads, Np));
  k.lws = w.take<char>(cs_ln_backward_workspace(M, C));
  k.tws = w.take<char>(cs_gemm_tn_workspace(M, C, C));
  k.end = w.end();
  return k;
}

// What a forward keeps for the backwards, in the handle's one kept region: x2 (M, C) fp32 | H (M, C) 16 bit | x1 (M, C) fp32 | x0 (M, C) fp32 |
// Os (M, C) 16 bit | lse_s (B, heads, Np) fp32, each from a 256-byte boundary.  A level's pieces are a prefix of the next level's; the pieces above
// `level` stay null.  The forward writes through this carve and the backwards read through it.
struct Kept { float* x2; h16_t* H; float *x1, *x0; h16_t* Os; float* lse_s; size_t end; };
inline Kept kept_carve(void* base, FitScope level, int B, int Np, int C, int heads) {
  const size_t mc = (size_t)B * Np * C;
  Carver w(base);
  Kept k{};
  if (level >= FIT_TAIL) { k.x2 = w.take<float>(mc * 4); k.H = w.take<h16_t>(mc * 2); }
  if (level >= FIT_CROSS) k.x1 = w.take<float>(mc * 4);
  if (level >= FIT_LAYER) {
    k.x0 = w.take<float>(mc * 4);
    k.Os = w.take<h16_t>(mc * 2);
    k.lse_s = w.take<float>((size_t)B * heads * Np * 4);
  }
  k.end = w.end();
  return k;
}

// out (M, C) = A (M, C) W^T + bias: the forward's GEMM on the square shapes of the backwards (W a packed weight, or a transposed copy of one)
inline CsGemmParams gemm_params(const h16_t* A, int lda, const h16_t* W, int ldw, int M, int C, const float* bias, void* out, int bf) {
  CsGemmParams g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = M; g.N = C; g.K = C; g.bias = bias; g.out = out; g.ldc = C; g.powp = 1.f; g.bf16 = bf;
  return g;
}

inline hipError_t gemm_go(const CsGemmParams& g, int epi, hipStream_t st) {
  if (cs_gemm_check(&g, epi)) return hipErrorInvalidValue;
  return cs_gemm_launch(&g, epi, st);
}

// ---- the block steps the scopes' launches are made of (host side; every one queues on st and waits for nothing) ----
// out (C, C) fp32 = (accumulate ? old : 0) + scale G (rows, C)^T X (rows, C), colsum (C) the column sums of G by the same rule
inline hipError_t reduce_tn(const h16_t* G, int ldg, const h16_t* X, int ldx, int rows, int C, float scale, int accumulate, float* out, float* colsum,
                            void* tws, int bf, hipStream_t st) {
  const CsGemmTn t{G, ldg, X, ldx, rows, C, C, scale, accumulate, out, C, colsum};
  return cs_gemm_tn_launch(&t, tws, bf, st);
}

// Through a weight: out (M, C) = G (M, C) W (+ resid), fp32 or 16 bit as the epilogue `epi` stores it.  The forward's GEMM multiplies by a transpose,
// so the packed W (C, ldw) is transposed into the scope's WT (stream order: the GEMM of its previous use has read it) and meets the zero bias zb.
inline hipError_t through_weight(const h16_t* G, const h16_t* W, int ldw, int M, int C, h16_t* WT, const float* zb, const float* resid, void* out,
                                 int epi, int bf, hipStream_t st) {
  hipError_t e = cs_transpose16_launch(W, ldw, C, C, WT, C, st);
  if (e != hipSuccess) return e;
  CsGemmParams g = gemm_params(G, C, WT, C, M, C, zb, out, bf);
  g.resid = resid; g.ldr = resid ? C : 0;
  return gemm_go(g, epi, st);
}

// The backward of a post-norm closing x = LayerNorm(y), y = resid + A W^T + b (norm3 behind H / W2, norm2 behind O / Wo, norm1 behind Os / Wo_s):
//   y recomputed (the forward never stores it)      (dgamma, dbeta, dyh) = ln_backward(y, dx, gamma)      db, dW = gemm_tn(dyh, A)      dA = dyh W (16 bit)
struct Closing { const h16_t* A; int lda; const h16_t* W; int ldw; const float* b; const float* resid; const float* gamma; float eps; };
struct ClosingWs { float* y; h16_t *dyh, *WT; const float* zb; void *lws, *tws; };                // the scope's workspace pieces
struct ClosingGrads { float *dW, *db, *dgamma, *dbeta; h16_t* dA; };                              // dA (M, C) stays in the workspace
inline hipError_t closing_backward(const Closing& c, const float* dx, const ClosingWs& w, const ClosingGrads& o, int M, int C, float scale,
                                   int accumulate, int bf, hipStream_t st) {
  hipError_t e;
  CsGemmParams gy = gemm_params(c.A, c.lda, c.W, c.ldw, M, C, c.b, w.y, bf);
  gy.resid = c.resid; gy.ldr = C;
  if ((e = gemm_go(gy, CS_EPI_RESID_F32, st)) != hipSuccess) return e;
  const CsLnBackward ln{w.y, C, dx, C, c.gamma, c.eps, M, C, scale, accumulate, w.dyh, C, o.dgamma, o.dbeta};
  if ((e = cs_ln_backward_launch(&ln, w.lws, bf, st)) != hipSuccess) return e;
  if ((e = reduce_tn(w.dyh, C, c.A, c.lda, M, C, scale, accumulate, o.dW, o.db, w.tws, bf, st)) != hipSuccess) return e;
  return through_weight(w.dyh, c.W, c.ldw, M, C, w.WT, w.zb, nullptr, o.dA, CS_EPI_BIAS_F16, bf, st);
}

// The attention backward of one block, on operands in place: Q (B Lq, ldq), K and V (B Lk, ldkv), O (B Lq, ldo), dO (B Lq, C) contiguous, lse
// (B, heads, Lq) base 2; the gradients dQ (B Lq, lddq), dK and dV (B Lk, lddkv).  A batch item's rows follow the previous item's everywhere.
inline CsAttnBwdParams attn_bwd_params(const h16_t* Q, int ldq, const h16_t* K, const h16_t* V, int ldkv, const h16_t* O, int ldo, const float* lse,
                                       const h16_t* dO, int B, int heads, int Lq, int Lk, int C, h16_t* dQ, int lddq, h16_t* dK, h16_t* dV,
                                       int lddkv, void* D, int bf) {
  CsAttnBwdParams a{};
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.dO = dO; a.lse = lse;
  a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = ldo; a.lddo = C;
  a.q_bs = (long long)Lq * ldq; a.k_bs = (long long)Lk * ldkv; a.v_bs = a.k_bs; a.o_bs = (long long)Lq * ldo; a.do_bs = (long long)Lq * C;
  a.nbatch = B; a.heads = heads; a.Lq = Lq; a.Lk = Lk; a.scale_log2e = 1.0f;
  a.dQ = dQ; a.lddq = lddq; a.dq_bs = (long long)Lq * lddq; a.dK = dK; a.dV = dV; a.lddk = a.lddv = lddkv; a.dk_bs = a.dv_bs = (long long)Lk * lddkv;
  a.D = static_cast<float*>(D); a.bf16 = bf;
  return a;
}

// The backward of an attention block behind its out_proj: the attention backward `a` (checked by the caller), the block's input rows x (M, C) fp32
// rounded into xh, then in_proj's three row blocks of dWin (3C, C) and dbin (3C): dQ against xh, dK and dV against the rows_k rows of Xk (the reference
// tokens, or xh itself).  The 1 / sqrt(dh) of the folded query scale and the ln2 of the base-2 logits ride in the reductions' fp32 scale.
inline hipError_t attn_block_backward(const CsAttnBwdParams& a, const float* x, h16_t* xh, int M, int C, const h16_t* Xk, int ldxk, int rows_k,
                                      float scale, int accumulate, float* dWin, float* dbin, void* tws, int bf, hipStream_t st) {
  const int dh = C / a.heads;
  const size_t cc = (size_t)C * C;
  hipError_t e;
  if ((e = cs_attnbwd_launch(&a, dh, st)) != hipSuccess) return e;
  if ((e = cs_pack_f16_launch(x, M, C, xh, C, nullptr, nullptr, bf, st)) != hipSuccess) return e;
  if ((e = reduce_tn(a.dQ, a.lddq, xh, C, M, C, scale * (1.0f / std::sqrt((float)dh)), accumulate, dWin, dbin, tws, bf, st)) != hipSuccess) return e;
  if ((e = reduce_tn(a.dK, a.lddk, Xk, ldxk, rows_k, C, scale * 0.69314718055994531f, accumulate, dWin + cc, dbin + C, tws, bf, st)) != hipSuccess) return e;
  return reduce_tn(a.dV, a.lddv, Xk, ldxk, rows_k, C, scale, accumulate, dWin + 2 * cc, dbin + 2 * C, tws, bf, st);
}

}  // namespace cs_fit
