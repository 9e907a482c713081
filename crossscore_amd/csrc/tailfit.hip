// Fitting the decoder's tail on the device: the backward of the last decoder layer's linear1 -> ReLU -> linear2 -> + residual
// -> norm3 in front of the head's (headfit.hip).  The forward is untouched; with cs_fit_tail_keep it leaves x2 (the last norm2 output, fp32) and
// H = relu(linear1(x2)) (16 bit) behind, and the head's backward leaves dpre (M, C) in its workspace.
//
//   dX = dpre Wa          the forward's GEMM over a transposed copy of the packed weight (cs_transpose16_launch), fp32 store
//   y = x2 + H W2^T + b2  the forward's GEMM with the residual epilogue: the pre-LayerNorm sum is recomputed, never stored by the forward
//   ln_backward           one wave per row, the row in registers (float4 per lane): mean and variance two-pass as layernorm_kernel has them,
//                         xhat, then dy = rstd (gamma dX - mean(gamma dX) - xhat mean(gamma dX xhat)) rounded once to the operand type.  A
//                         workgroup owns CS_TAILFIT_LN_ROW_TILE rows: each wave adds dX xhat and dX over its rows in row order in registers,
//                         the waves' sums are added through LDS in wave order into one fp32 partial row each, and ln_reduce adds the
//                         partials in workgroup order.  No atomics: two runs give the same bits.
//   dH = dyh W2           the same transposed-weight GEMM with a 16-bit store, then relu_mask: dH * [H > 0] in place
//   dW2, db2, dW1, db1    gemm_tn (headfit.hip) over (dyh, H) and (dHh, x2 rounded to the operand type)
#include "fit_shared.h"

namespace {

using namespace cs_fit;

constexpr int LNB_ROWS = CS_TAILFIT_LN_ROW_TILE;  // rows of one workgroup

__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// V float4 per lane (C <= 256 V); NW waves share the workgroup's CS_TAILFIT_LN_ROW_TILE rows, consecutive runs of LNB_ROWS / NW each.  A wave has
// the next row's loads in flight while it works on the current one: with four reductions in a chain per row the kernel is bound by latency,
// not by its 5 bytes per element.
template <int V, int NW, bool BF> __global__ __launch_bounds__(64 * NW) void ln_backward_kernel(CsLnBackward p, float* part) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [NW waves][2][C]
  constexpr int WROWS = LNB_ROWS / NW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = p.C, C4 = C / 4, M = p.M;
  const float* const ybase = p.y; const float* const dbase = p.dx;
  const size_t ldy = p.ldy, ldx = p.ldx;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gam[V], ag[V], ab[V], yn[V], dn[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = lane + i * 64;
    gam[i] = zero4; ag[i] = zero4; ab[i] = zero4;
    if (c < C4) gam[i] = reinterpret_cast<const float4*>(p.gamma)[c];  // (an `in ? load : zero4` selects between ADDRESSES: zero4 in scratch, flat loads)
  }
  const int r0 = blockIdx.x * LNB_ROWS + wave * WROWS;
#define LNB_FETCH(m_)  /* rows past M are neither read nor written */ \
  _Pragma("unroll") for (int i = 0; i < V; ++i) {                       \
    const int c = lane + i * 64;                                        \
    const bool in = (m_) < M && c < C4;                                 \
    yn[i] = zero4; dn[i] = zero4;                                       \
    if (in) {                                                           \
      yn[i] = reinterpret_cast<const float4*>(ybase + (size_t)(m_) * ldy)[c]; \
      dn[i] = reinterpret_cast<const float4*>(dbase + (size_t)(m_) * ldx)[c]; \
    }                                                                   \
  }
  LNB_FETCH(r0)
  for (int r = 0; r < WROWS; ++r) {
    const int m = r0 + r;
    if (m >= M) break;  // (wave-uniform)
    float4 y[V], d[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      y[i] = yn[i]; d[i] = dn[i];
      s += sum4(y[i]);
    }
    if (r + 1 < WROWS) { LNB_FETCH(m + 1) }
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool in = lane + i * 64 < C4;
      y[i].x = in ? y[i].x - mu : 0.f; y[i].y = in ? y[i].y - mu : 0.f; y[i].z = in ? y[i].z - mu : 0.f; y[i].w = in ? y[i].w - mu : 0.f;
      q += (y[i].x * y[i].x + y[i].y * y[i].y) + (y[i].z * y[i].z + y[i].w * y[i].w);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + p.eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      y[i].x *= rstd; y[i].y *= rstd; y[i].z *= rstd; y[i].w *= rstd;  // xhat (zero past C)
      const float4 gd = make_float4(gam[i].x * d[i].x, gam[i].y * d[i].y, gam[i].z * d[i].z, gam[i].w * d[i].w);
      s1 += sum4(gd);
      s2 += (gd.x * y[i].x + gd.y * y[i].y) + (gd.z * y[i].z + gd.w * y[i].w);
    }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    h16_t* orow = p.dyh + (size_t)m * p.ldd;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int c = lane + i * 64;
      if (c < C4) {
        uint2 o;
        o.x = pack_o16x2<BF>(rstd * (gam[i].x * d[i].x - m1 - y[i].x * m2), rstd * (gam[i].y * d[i].y - m1 - y[i].y * m2));
        o.y = pack_o16x2<BF>(rstd * (gam[i].z * d[i].z - m1 - y[i].z * m2), rstd * (gam[i].w * d[i].w - m1 - y[i].w * m2));
        reinterpret_cast<uint2*>(orow)[c] = o;
      }
      ag[i].x += d[i].x * y[i].x; ag[i].y += d[i].y * y[i].y; ag[i].z += d[i].z * y[i].z; ag[i].w += d[i].w * y[i].w;
      ab[i].x += d[i].x; ab[i].y += d[i].y; ab[i].z += d[i].z; ab[i].w += d[i].w;
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = lane + i * 64;
    if (c < C4) {
      reinterpret_cast<float4*>(red + (size_t)(wave * 2) * C)[c] = ag[i];
      reinterpret_cast<float4*>(red + (size_t)(wave * 2 + 1) * C)[c] = ab[i];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * C; idx += 64 * NW) {  // idx = which * C + c; the waves' sums in wave order
    float t = red[idx];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += red[(size_t)w * 2 * C + idx];
    part[(size_t)blockIdx.x * 2 * C + idx] = t;
  }
#undef LNB_FETCH
}

// dgamma / dbeta = (accumulate ? old : 0) + scale * (the workgroups' partial rows in workgroup order; 32 loads in flight, the adds in order)
__global__ void ln_reduce_kernel(const float* part, int nwg, int C, float scale, int accumulate, float* dgamma, float* dbeta) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  const size_t step = (size_t)2 * C;
  const float* src = part + idx;
  float s = 0.f;
  int w = 0;
  for (; w + 32 <= nwg; w += 32) {
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = src[(size_t)(w + i) * step];
#pragma unroll
    for (int i = 0; i < 32; ++i) s += v[i];
  }
  for (; w < nwg; ++w) s += src[(size_t)w * step];
  float* o = idx < C ? dgamma + idx : dbeta + (idx - C);
  *o = (accumulate ? *o : 0.f) + scale * s;
}

// dH (M, C; contiguous) *= [H > 0] in place, eight elements per thread: the mask reads the stored activation's bits, 0 and -0 take 0
__global__ void relu_mask_kernel(h16_t* dH, const h16_t* H, int ldh, int M, int C8) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)M * C8) return;
  const int m = (int)(idx / C8), c8 = (int)(idx - (long long)m * C8);
  uint4* dp = reinterpret_cast<uint4*>(dH) + idx;
  const uint4 h = *reinterpret_cast<const uint4*>(H + (size_t)m * ldh + (size_t)c8 * 8);
  uint4 d = *dp;
  auto keep = [](uint32_t hw) {  // per 16-bit half: all ones where the half is a positive number
    const uint32_t lo = hw & 0xFFFFu, hi = hw >> 16;
    return ((!(lo & 0x8000u) && (lo & 0x7FFFu)) ? 0xFFFFu : 0u) | ((!(hi & 0x8000u) && (hi & 0x7FFFu)) ? 0xFFFF0000u : 0u);
  };
  d.x &= keep(h.x); d.y &= keep(h.y); d.z &= keep(h.z); d.w &= keep(h.w);
  *dp = d;
}

template <int V, int NW> hipError_t ln_backward_go(const CsLnBackward& p, float* part, int nwg, int bf, hipStream_t st) {
  const size_t lds = (size_t)NW * 2 * p.C * sizeof(float);  // at most 64 KiB: 8 waves x 2 x 512 or 4 waves x 2 x 2048 floats
  if (bf) ln_backward_kernel<V, NW, true><<<nwg, 64 * NW, lds, st>>>(p, part);
  else ln_backward_kernel<V, NW, false><<<nwg, 64 * NW, lds, st>>>(p, part);
  return hipGetLastError();
}

}  // namespace

extern "C" {

size_t cs_ln_backward_workspace(int M, int C) { return up256((size_t)((M + LNB_ROWS - 1) / LNB_ROWS) * 2 * C * sizeof(float)); }

hipError_t cs_ln_backward_launch(const CsLnBackward* p, void* ws, int bf, hipStream_t st) {
  const int nwg = (p->M + LNB_ROWS - 1) / LNB_ROWS;
  float* part = static_cast<float*>(ws);
  hipError_t e;
  // eight waves of four rows where the row is short (the decoder widths of the tiny and ViT-S nets), four waves of eight rows above
  if (p->C <= 256) e = ln_backward_go<1, 8>(*p, part, nwg, bf, st);
  else if (p->C <= 512) e = ln_backward_go<2, 8>(*p, part, nwg, bf, st);
  else if (p->C <= 1024) e = ln_backward_go<4, 4>(*p, part, nwg, bf, st);
  else e = ln_backward_go<8, 4>(*p, part, nwg, bf, st);
  if (e != hipSuccess) return e;
  ln_reduce_kernel<<<(2 * p->C + 255) / 256, 256, 0, st>>>(part, nwg, p->C, p->scale, p->accumulate, p->dgamma, p->dbeta);
  return hipGetLastError();
}

// the workspace of one whole tail backward: tail_carve (fit_shared.h), which the launch below takes its pointers from.  dyh and dH (M, C; 16 bit,
// contiguous) stay in it: the cross-attention fit continues from them
size_t cs_tail_backward_workspace(int M, int C) { return tail_carve(nullptr, M, C).end; }

hipError_t cs_tail_backward_launch(const CsTailBackward* q, void* ws, int bf, hipStream_t st) {
  const CsHeadBackward& hq = q->head;
  const int M = hq.B * hq.gh * hq.gw, C = hq.C;
  const TailWs k = tail_carve(ws, M, C);
  const float scale = (float)hq.inv_count;
  hipError_t e = cs_head_backward_launch(&hq, ws, bf, st);  // dWa, dba, dWb, dbb, the loss; dpre stays in the workspace
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(k.zb, 0, (size_t)C * 4, st)) != hipSuccess) return e;
  // dX = dpre Wa
  if ((e = through_weight(k.head.dpre, q->Wa, q->ldwa, M, C, k.WT, k.zb, nullptr, k.dX, CS_EPI_RESID_F32, bf, st)) != hipSuccess) return e;
  // y = x2 + H W2^T + b2 and norm3: dg3, db3, dyh; dW2, db2; dH = dyh W2
  const Closing c{q->H, q->ldh, q->W2, q->ldw2, q->b2, q->x2, q->gamma3, q->eps};
  if ((e = closing_backward(c, k.dX, {k.y, k.dyh, k.WT, k.zb, k.lws, k.tws}, {q->dW2, q->db2, q->dg3, q->db3, k.dH}, M, C, scale, hq.accumulate, bf, st)) !=
      hipSuccess)
    return e;
  // dHh = dH * [H > 0], then dW1, db1 against x2 rounded to the operand type
  const long long n8 = (long long)M * (C / 8);
  relu_mask_kernel<<<(unsigned)((n8 + 255) / 256), 256, 0, st>>>(k.dH, q->H, q->ldh, M, C / 8);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = cs_pack_f16_launch(q->x2, M, C, k.x2h, C, nullptr, nullptr, bf, st)) != hipSuccess) return e;
  return reduce_tn(k.dH, C, k.x2h, C, M, C, scale, hq.accumulate, q->dW1, q->db1, k.tws, bf, st);
}

}
