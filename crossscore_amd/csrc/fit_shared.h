// What headfit.hip, tailfit.hip, crossfit.hip and layerfit.hip share: the 256-byte rounding, the square GEMM of the transposed-weight
// trick, and ONE carve per backward workspace.  The scopes are nested -- the tail's workspace begins with the head's, the cross-attention fit's with
// the tail's, the whole layer's with the cross-attention fit's -- and so are the carves: a launch reads its parent's pieces (dpre; dyh and dH; dy2h
// and dQu) from the parent's carve.  `end` is the workspace's size
// in bytes, so the size a caller allocates by is the carve over a null base that the launch takes its pointers from.
#pragma once
#include "cs_common.h"

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

}  // namespace cs_fit
