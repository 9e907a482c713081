// Whole-layer fit: the backward of the last decoder layer's self-attention block -- in_proj, attention, out_proj, the residual
// and norm1 -- in front of the cross-attention fit's (crossfit.hip), composed from the operators that exist: the cross backward (which leaves dy2h
// and dQu in its workspace), the GEMM with fp32 / 16-bit stores and the transposed-weight trick, ln_backward, gemm_tn with its column sums, and the
// attention backward (attnbwd.hip) on the packed Q' | K | V rows in place.  The only kernel of its own closes dx1 in fp32.
//   dx1 = (short cut ? f32(dy2h) : 0) + ln2 dQu Wq'      y1 = (short cut ? x0 : 0) + Os Wo_s^T + bo_s      (dgamma1, dbeta1, dy1h) = ln_backward(y1, dx1, gamma1)
//   dbo_s, dWo_s = gemm_tn(dy1h, Os)      dOsh = dy1h Wo_s (16 bit)      (dQu_s | dKu_s | dV_s) = attention backward, Lq = Lk = Np per batch item
//   in_proj rows [0, C): gemm_tn(dQu_s, x0h) scaled inv_count / sqrt(dh);  [C, 2C): gemm_tn(dKu_s, x0h) scaled inv_count ln2;  [2C, 3C): gemm_tn(dV_s, x0h)
// d loss / d Q' = ln2 dQu (f17's scalars) and Wq' carries the folded query scale, so dx1 needs no factor beyond the ln2.  The GEMM's epilogues
// take no per-column scale (cs_gemm_check refuses one: the forward folds its scales into the packed weights), so the product is stored in fp32 and
// dx1_close_kernel applies the ln2 and adds the residual gradient there: the ln2 never meets a 16-bit value.
// The gradient stops at x0.  Every sum has a fixed order; nothing is accumulated with atomics.
#include "fit_shared.h"

namespace {

using namespace cs_fit;

constexpr float kLn2 = 0.69314718055994531f;

// g (n) fp32 = ln2 g + (r ? the values of r's 16-bit elements : 0), eight per thread (n a multiple of 8)
__global__ void dx1_close_kernel(float* g, const h16_t* r, long long n8, int bf) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float4 lo = reinterpret_cast<const float4*>(g)[2 * i], hi = reinterpret_cast<const float4*>(g)[2 * i + 1];
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r) {
    const uint4 v = reinterpret_cast<const uint4*>(r)[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[2 * j] = o2f((h16_t)(w[j] & 0xffffu), bf); a[2 * j + 1] = o2f((h16_t)(w[j] >> 16), bf); }
  }
  lo.x = fmaf(kLn2, lo.x, a[0]); lo.y = fmaf(kLn2, lo.y, a[1]); lo.z = fmaf(kLn2, lo.z, a[2]); lo.w = fmaf(kLn2, lo.w, a[3]);
  hi.x = fmaf(kLn2, hi.x, a[4]); hi.y = fmaf(kLn2, hi.y, a[5]); hi.z = fmaf(kLn2, hi.z, a[6]); hi.w = fmaf(kLn2, hi.w, a[7]);
  reinterpret_cast<float4*>(g)[2 * i] = lo;
  reinterpret_cast<float4*>(g)[2 * i + 1] = hi;
}

LayerWs layer_carve(const CsLayerBackward* q, void* ws) {
  const CsHeadBackward& hq = q->cross.tail.head;
  return cs_fit::layer_carve(ws, hq.B, hq.gh * hq.gw, q->cross.N, hq.C, q->cross.heads);
}

}  // namespace

extern "C" {

size_t cs_layer_backward_workspace(int B, int Np, int N, int C, int heads) { return cs_fit::layer_carve(nullptr, B, Np, N, C, heads).end; }

// The self-attention backward of one layer backward, as the launch below queues it: Q', K and V in place in their packed rows, every batch item
// attending to its own Np keys, dQu_s | dKu_s | dV_s side by side.  layer_backward_run (fit_host.hip) builds it too and puts it through
// cs_attnbwd_check with every other check, before the first launch.
void cs_layer_backward_attn_params(const CsLayerBackward* q, void* ws, int bf, CsAttnBwdParams* out) {
  const CsHeadBackward& hq = q->cross.tail.head;
  const int B = hq.B, Np = hq.gh * hq.gw, C = hq.C;
  const LayerWs k = layer_carve(q, ws);
  *out = attn_bwd_params(q->Qs, q->ldqkv, q->Ks, q->Vs, q->ldqkv, q->Os, q->ldos, q->lse_s, k.dOsh, B, q->cross.heads, Np, Np, C, k.dQKV, 3 * C,
                         k.dQKV + C, k.dQKV + 2 * C, 3 * C, k.aws, bf);
}

hipError_t cs_layer_backward_launch(const CsLayerBackward* q, void* ws, int bf, hipStream_t st) {
  const CsCrossBackward& x = q->cross;
  const CsHeadBackward& hq = x.tail.head;
  const int M = hq.B * hq.gh * hq.gw, C = hq.C;
  const LayerWs k = layer_carve(q, ws);
  const float scale = (float)hq.inv_count;
  hipError_t e = cs_cross_backward_launch(&x, ws, bf, st);  // the sixteen gradients of the three inner scopes, the loss; dy2h and dQu stay in the workspace
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(k.zb, 0, (size_t)C * 4, st)) != hipSuccess) return e;
  // dx1 = (short cut ? f32(dy2h) : 0) + ln2 dQu Wq'
  if ((e = through_weight(k.dQu, q->Wq, q->ldwq, M, C, k.WT, k.zb, nullptr, k.dx1, CS_EPI_RESID_F32, bf, st)) != hipSuccess) return e;
  const long long n8 = (long long)((size_t)M * C / 8);
  dx1_close_kernel<<<(unsigned)((n8 + 255) / 256), 256, 0, st>>>(k.dx1, x.short_cut ? k.dy2h : nullptr, n8, bf);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // y1 = (short cut ? x0 : 0) + Os Wo_s^T + bo_s and norm1: dg1, db1, dy1h; dWo_s, dbo_s; dOsh = dy1h Wo_s
  const Closing c{q->Os, q->ldos, q->Wo_s, q->ldwos, q->bo_s, x.short_cut ? q->x0 : nullptr, q->gamma1, x.tail.eps};
  if ((e = closing_backward(c, k.dx1, {k.y1, k.dy1h, k.WT, k.zb, k.lws, k.tws}, {q->dWo_s, q->dbo_s, q->dg1, q->db1, k.dOsh}, M, C, scale, hq.accumulate,
                            bf, st)) != hipSuccess)
    return e;
  // the self-attention backward (its parameters: cs_layer_backward_attn_params above) and in_proj: all three blocks against x0h, the one rounding of x0
  CsAttnBwdParams a{};
  cs_layer_backward_attn_params(q, ws, bf, &a);
  return attn_block_backward(a, q->x0, k.x0h, M, C, k.x0h, C, M, scale, hq.accumulate, q->dWin_s, q->dbin_s, k.tws, bf, st);
}

}
