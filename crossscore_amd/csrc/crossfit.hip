// Cross-attention fit: the backward of the last decoder layer's cross-attention block -- in_proj, attention, out_proj, the
// residual and norm2 -- in front of the tail's (tailfit.hip), composed from the operators that exist: the tail's backward (which leaves dyh and
// dHh in its workspace), the GEMM with fp32 / 16-bit stores and the transposed-weight trick, ln_backward, gemm_tn with its column sums, and the
// attention backward (attnbwd.hip).  The only kernel of its own widens 16-bit rows to fp32.
//   dx2 = f32(dyh) + dHh W1          y2 = (short cut ? x1 : 0) + O Wo^T + bo          (dgamma2, dbeta2, dy2h) = ln_backward(y2, dx2, gamma2)
//   dbo, dWo = gemm_tn(dy2h, O)      dOh = dy2h Wo (16 bit)      (dQu, dKu | dV) = attention backward
//   in_proj rows [0, C): gemm_tn(dQu, x1h) scaled inv_count / sqrt(dh);  [C, 2C): gemm_tn(dKu, mem) scaled inv_count ln2;  [2C, 3C): gemm_tn(dV, mem)
// Every sum has a fixed order; nothing is accumulated with atomics.
#include "fit_shared.h"

#include <cmath>

namespace {

using namespace cs_fit;

// out (n) fp32 = the values of the 16-bit elements, eight per thread (n a multiple of 8)
__global__ void widen16_kernel(const h16_t* src, float* out, long long n8, int bf) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const uint4 v = reinterpret_cast<const uint4*>(src)[i];
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float4 lo, hi;
  lo.x = o2f((h16_t)(w[0] & 0xffffu), bf); lo.y = o2f((h16_t)(w[0] >> 16), bf); lo.z = o2f((h16_t)(w[1] & 0xffffu), bf); lo.w = o2f((h16_t)(w[1] >> 16), bf);
  hi.x = o2f((h16_t)(w[2] & 0xffffu), bf); hi.y = o2f((h16_t)(w[2] >> 16), bf); hi.z = o2f((h16_t)(w[3] & 0xffffu), bf); hi.w = o2f((h16_t)(w[3] >> 16), bf);
  reinterpret_cast<float4*>(out)[2 * i] = lo;
  reinterpret_cast<float4*>(out)[2 * i + 1] = hi;
}

// the pieces of one whole backward's workspace (cs_fit::cross_carve, fit_shared.h) for the launch, for the parameters its caller checks and for the size
CrossWs cross_carve(const CsCrossBackward* q, void* ws) {
  const CsHeadBackward& hq = q->tail.head;
  return cs_fit::cross_carve(ws, hq.B, hq.gh * hq.gw, q->N, hq.C, q->heads);
}

}  // namespace

extern "C" {

size_t cs_cross_backward_workspace(int B, int Np, int N, int C, int heads) { return cs_fit::cross_carve(nullptr, B, Np, N, C, heads).end; }

// The attention backward of one cross backward, as the launch below queues it: K and V in place in their packed rows, dKu | dV side by side.
// cross_backward_run (ops.hip) builds it too and puts it through cs_attnbwd_check with every other check, before the first launch.
void cs_cross_backward_attn_params(const CsCrossBackward* q, void* ws, int bf, CsAttnBwdParams* out) {
  const CsHeadBackward& hq = q->tail.head;
  const int B = hq.B, Np = hq.gh * hq.gw, C = hq.C;
  const CrossWs k = cross_carve(q, ws);
  CsAttnBwdParams a{};
  a.Q = q->Qp; a.K = q->K; a.V = q->V; a.O = q->O; a.dO = k.dOh; a.lse = q->lse;
  a.ldq = q->ldq; a.ldk = q->ldkv; a.ldv = q->ldkv; a.ldo = q->ldo; a.lddo = C;
  a.q_bs = (long long)Np * q->ldq; a.k_bs = (long long)q->N * Np * q->ldkv; a.v_bs = a.k_bs; a.o_bs = (long long)Np * q->ldo; a.do_bs = (long long)Np * C;
  a.nbatch = B; a.heads = q->heads; a.Lq = Np; a.Lk = q->N * Np; a.scale_log2e = 1.0f;
  a.dQ = k.dQu; a.lddq = C; a.dq_bs = (long long)Np * C;
  a.dK = k.dKV; a.lddk = 2 * C; a.dk_bs = (long long)q->N * Np * 2 * C;
  a.dV = k.dKV + C; a.lddv = 2 * C; a.dv_bs = a.dk_bs;
  a.D = static_cast<float*>(k.aws); a.bf16 = bf;
  *out = a;
}

hipError_t cs_cross_backward_launch(const CsCrossBackward* q, void* ws, int bf, hipStream_t st) {
  const CsHeadBackward& hq = q->tail.head;
  const int B = hq.B, Np = hq.gh * hq.gw, M = B * Np, Mk = M * q->N, C = hq.C, dh = C / q->heads;
  const size_t mc = (size_t)M * C;
  const CrossWs k = cross_carve(q, ws);
  const h16_t *dyh = k.dyh, *dHh = k.dHh;
  h16_t *WT = k.WT, *dy2h = k.dy2h, *dOh = k.dOh, *x1h = k.x1h, *dQu = k.dQu, *dKV = k.dKV;
  float *zb = k.zb, *dyf = k.dyf, *dx2 = k.dx2, *y2 = k.y2;
  void *lws = k.lws, *tws = k.tws;
  const float scale = (float)hq.inv_count;
  hipError_t e = cs_tail_backward_launch(&q->tail, ws, bf, st);  // the ten gradients of the tail and the head, the loss; dyh and dHh stay in the workspace
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(zb, 0, (size_t)C * 4, st)) != hipSuccess) return e;
  // dx2 = f32(dyh) + dHh W1
  const long long n8 = (long long)(mc / 8);
  widen16_kernel<<<(unsigned)((n8 + 255) / 256), 256, 0, st>>>(dyh, dyf, n8, bf);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = cs_transpose16_launch(q->W1, q->ldw1, C, C, WT, C, st)) != hipSuccess) return e;
  CsGemmParams gx = gemm_params(dHh, C, WT, C, M, C, zb, dx2, bf);
  gx.resid = dyf; gx.ldr = C;
  if ((e = gemm_go(gx, CS_EPI_RESID_F32, st)) != hipSuccess) return e;
  // y2 = (short cut ? x1 : 0) + O Wo^T + bo
  CsGemmParams gy = gemm_params(q->O, q->ldo, q->Wo, q->ldwo, M, C, q->bo, y2, bf);
  gy.resid = q->short_cut ? q->x1 : nullptr; gy.ldr = C;
  if ((e = gemm_go(gy, CS_EPI_RESID_F32, st)) != hipSuccess) return e;
  CsLnBackward ln{};
  ln.y = y2; ln.ldy = C; ln.dx = dx2; ln.ldx = C; ln.gamma = q->gamma2; ln.eps = q->tail.eps; ln.M = M; ln.C = C; ln.scale = scale; ln.accumulate = hq.accumulate;
  ln.dyh = dy2h; ln.ldd = C; ln.dgamma = q->dg2; ln.dbeta = q->db2;
  if ((e = cs_ln_backward_launch(&ln, lws, bf, st)) != hipSuccess) return e;
  // dWo, dbo
  CsGemmTn t{};
  t.G = dy2h; t.ldg = C; t.X = q->O; t.ldx = q->ldo; t.M = M; t.N = C; t.K = C; t.scale = scale; t.accumulate = hq.accumulate;
  t.out = q->dWo; t.ldo = C; t.colsum = q->dbo;
  if ((e = cs_gemm_tn_launch(&t, tws, bf, st)) != hipSuccess) return e;
  // dOh = dy2h Wo
  if ((e = cs_transpose16_launch(q->Wo, q->ldwo, C, C, WT, C, st)) != hipSuccess) return e;  // (stream order: dx2's GEMM has read WT)
  if ((e = gemm_go(gemm_params(dy2h, C, WT, C, M, C, zb, dOh, bf), CS_EPI_BIAS_F16, st)) != hipSuccess) return e;
  // the attention backward (its parameters: cs_cross_backward_attn_params above; checked by the caller with everything else)
  CsAttnBwdParams a{};
  cs_cross_backward_attn_params(q, ws, bf, &a);
  if ((e = cs_attnbwd_launch(&a, dh, st)) != hipSuccess) return e;
  // in_proj: the 1 / sqrt(dh) of the folded query scale and the ln2 of the base-2 logits ride in the reductions' fp32 scale
  if ((e = cs_pack_f16_launch(q->x1, M, C, x1h, C, nullptr, nullptr, bf, st)) != hipSuccess) return e;
  t.G = dQu; t.ldg = C; t.X = x1h; t.ldx = C; t.M = M; t.scale = scale * (1.0f / std::sqrt((float)dh)); t.out = q->dWin; t.colsum = q->dbin;
  if ((e = cs_gemm_tn_launch(&t, tws, bf, st)) != hipSuccess) return e;
  t.G = dKV; t.ldg = 2 * C; t.X = q->mem; t.ldx = q->ldm; t.M = Mk; t.scale = scale * 0.69314718055994531f; t.out = q->dWin + (size_t)C * C; t.colsum = q->dbin + C;
  if ((e = cs_gemm_tn_launch(&t, tws, bf, st)) != hipSuccess) return e;
  t.G = dKV + C; t.scale = scale; t.out = q->dWin + (size_t)2 * C * C; t.colsum = q->dbin + 2 * C;
  return cs_gemm_tn_launch(&t, tws, bf, st);
}

}
