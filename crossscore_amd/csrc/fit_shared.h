// What headfit.hip, tailfit.hip and crossfit.hip share: the 256-byte rounding, the square GEMM of the transposed-weight trick, and
// ONE carve per backward workspace.  The scopes are nested -- the tail's workspace begins with the head's, the cross-attention fit's with the
// tail's -- and so are the carves: a launch reads its parent's pieces (dpre; dyh and dH) from the parent's carve.  `end` is the workspace's size
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
