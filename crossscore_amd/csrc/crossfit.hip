// Cross-attention fit: the backward of the last decoder layer's cross-attention block -- in_proj, attention, out_proj, the
// residual and norm2 -- in front of the tail's (tailfit.hip), composed from the operators that exist: the tail's backward (which leaves dyh and
// dHh in its workspace), the GEMM with fp32 / 16-bit stores and the transposed-weight trick, ln_backward, gemm_tn with its column sums, and the
// attention backward (attnbwd.hip).  The only kernel of its own widens 16-bit rows to fp32.
//   dx2 = f32(dyh) + dHh W1          y2 = (short cut ? x1 : 0) + O Wo^T + bo          (dgamma2, dbeta2, dy2h) = ln_backward(y2, dx2, gamma2)
//   dbo, dWo = gemm_tn(dy2h, O)      dOh = dy2h Wo (16 bit)      (dQu, dKu | dV) = attention backward
//   in_proj rows [0, C): gemm_tn(dQu, x1h) scaled inv_count / sqrt(dh);  [C, 2C): gemm_tn(dKu, mem) scaled inv_count ln2;  [2C, 3C): gemm_tn(dV, mem)
// Every sum has a fixed order; nothing is accumulated with atomics.
#include "fit_shared.h"

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
// cross_backward_run (fit_host.hip) builds it too and puts it through cs_attnbwd_check with every other check, before the first launch.
void cs_cross_backward_attn_params(const CsCrossBackward* q, void* ws, int bf, CsAttnBwdParams* out) {
  const CsHeadBackward& hq = q->tail.head;
  const int B = hq.B, Np = hq.gh * hq.gw, C = hq.C;
  const CrossWs k = cross_carve(q, ws);
  *out = attn_bwd_params(q->Qp, q->ldq, q->K, q->V, q->ldkv, q->O, q->ldo, q->lse, k.dOh, B, q->heads, Np, q->N * Np, C, k.dQu, C, k.dKV, k.dKV + C,
                         2 * C, k.aws, bf);
}

hipError_t cs_cross_backward_launch(const CsCrossBackward* q, void* ws, int bf, hipStream_t st) {
  const CsHeadBackward& hq = q->tail.head;
  const int M = hq.B * hq.gh * hq.gw, Mk = M * q->N, C = hq.C;
  const CrossWs k = cross_carve(q, ws);
  const float scale = (float)hq.inv_count;
  hipError_t e = cs_tail_backward_launch(&q->tail, ws, bf, st);  // the ten gradients of the tail and the head, the loss; dyh and dHh stay in the workspace
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(k.zb, 0, (size_t)C * 4, st)) != hipSuccess) return e;
  // dx2 = f32(dyh) + dHh W1
  const long long n8 = (long long)((size_t)M * C / 8);
  widen16_kernel<<<(unsigned)((n8 + 255) / 256), 256, 0, st>>>(k.dyh, k.dyf, n8, bf);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = through_weight(k.dHh, q->W1, q->ldw1, M, C, k.WT, k.zb, k.dyf, k.dx2, CS_EPI_RESID_F32, bf, st)) != hipSuccess) return e;
  // y2 = (short cut ? x1 : 0) + O Wo^T + bo and norm2: dg2, db2, dy2h; dWo, dbo; dOh = dy2h Wo
  const Closing c{q->O, q->ldo, q->Wo, q->ldwo, q->bo, q->short_cut ? q->x1 : nullptr, q->gamma2, q->tail.eps};
  if ((e = closing_backward(c, k.dx2, {k.y2, k.dy2h, k.WT, k.zb, k.lws, k.tws}, {q->dWo, q->dbo, q->dg2, q->db2, k.dOh}, M, C, scale, hq.accumulate, bf,
                            st)) != hipSuccess)
    return e;
  // the attention backward (its parameters: cs_cross_backward_attn_params above) and in_proj: dQu against x1h, dKu | dV against the reference tokens
  CsAttnBwdParams a{};
  cs_cross_backward_attn_params(q, ws, bf, &a);
  return attn_block_backward(a, q->x1, k.x1h, M, C, q->mem, q->ldm, Mk, scale, hq.accumulate, q->dWin, q->dbin, k.tws, bf, st);
}

}
