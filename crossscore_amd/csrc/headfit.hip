// Fitting the regression head on the device: the L1 loss of the score map against a ground-truth map, its gradient through
// sigmoid | tanh -> pow -> jigsaw and the head's two linears, and AdamW.  The forward is untouched; these kernels read what it left behind
// (the 16-bit tokens X behind the last norm3 and the hidden rows A = leaky(X Wa^T + ba)) and the packed second linear Wb.
//
//   head_grad_z   z = A Wb^T + bb (MFMA 16x16x32, both operands k-contiguous, fragments straight from global memory: Wb is 150 KB and stays in
//                 L2), then per element sigma, s = sigma^p, gt through the jigsaw, |s - gt| into an fp64 partial, g = sign(s - gt) ds/dz rounded
//                 ONCE to the operand type.  g has HF_NP = 224 columns: 196 padded with zeros to whole 32-deep k steps of the dA product.
//   head_da       dpre = (g Wb) * (A > 0 ? 1 : 0.01), rounded once; Wb arrives as a transposed, zero-padded 16-bit copy (hf_transpose) so that
//                 this product has k-contiguous operands too.
//   gemm_tn       out (N, K) = scale * sum_m G[m][n] X[m][k]: both operands have the summed index as their row, so 32-row tiles of both go
//                 through LDS and the fragments are read with ds_read_b64_tr_b16.  Rows are split into fixed chunks of HF_CHUNK; every
//                 chunk writes an fp32 partial and a second kernel adds the partials in chunk order.  The same pair of kernels sums G's columns
//                 (the bias gradients).  No atomics anywhere: two runs give the same bits.
//   adamw         torch.optim.AdamW's single-tensor step in fp32, optionally with the parameter's 16-bit operand copy in the same pass.
#include "fit_shared.h"
#include <cmath>

namespace {

using namespace cs_fit;

constexpr int HF_ROWS = CS_HEADFIT_ROW_TILE;   // rows of one workgroup of head_grad_z / head_da: 4 waves x 16
constexpr int HF_NP = CS_HEADFIT_NPAD;         // g's columns: P*P = 196 padded to whole 32-deep k steps
constexpr int HF_CHUNK = CS_HEADFIT_ROW_CHUNK; // rows of one gemm_tn partial
constexpr int HF_LROW = 72;                    // LDS row of a 64-column tile in elements (144 B: 16-byte chunks stay aligned)

__device__ __forceinline__ h16x8_t frag_load(const h16_t* p, bool ok) {
  h16x8_t z = {};
  return ok ? *reinterpret_cast<const h16x8_t*>(p) : z;
}

// ---- z = A Wb^T + bb -> g, loss partial, column-sum partial ----
template <bool BF> __global__ __launch_bounds__(256) void head_grad_z_kernel(CsHeadGradZ p, double* loss_part) {
  __shared__ float red[4][HF_NP];
  __shared__ double lred[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int M = p.B * p.gh * p.gw, PP = p.P * p.P;
  const int m0 = blockIdx.x * HF_ROWS + wave * 16;
  constexpr int NT = 13;  // 16-column tiles that hold real columns (196 <= 208); the 14th is padding only
  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int ma = m0 + fr;
  const h16_t* arow = p.A + (size_t)(ma < M ? ma : 0) * p.lda + 8 * fq;
  for (int k0 = 0; k0 < p.C; k0 += 32) {
    const h16x8_t a = frag_load(arow + k0, ma < M);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 16 + fr;
      const h16x8_t b = frag_load(p.Wb + (size_t)(n < PP ? n : 0) * p.ldw + k0 + 8 * fq, n < PP);
      acc[t] = mfma_16x16x32<BF>(a, b, acc[t]);
    }
  }
  const int Np = p.gh * p.gw, Wimg = p.gw * p.P;
  double lsum = 0.0;
#pragma unroll
  for (int t = 0; t < NT + 1; ++t) {
    const int n = t * 16 + fr;
    float csum = 0.f;
    if (t < NT && n < PP) {
      const int py = n / p.P, px = n - py * p.P;
      const float bias = p.bb[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + fq * 4 + r;
        if (m >= M) continue;
        const int b = m / Np, rem = m - b * Np, i = rem / p.gw, j = rem - i * p.gw;
        const float z = acc[t < NT ? t : 0][r] + bias;
        const float sg = p.act == 0 ? 1.0f / (1.0f + __expf(-z)) : tanhf(z);
        const float s = p.powp != 1.0f ? powf(sg, p.powp) : sg;
        float ds;  // ds/dz
        if (p.act == 0) ds = p.powp * s * (1.0f - sg);  // p sigma^(p-1) * sigma (1 - sigma)
        else ds = 1.0f - sg * sg;  // tanh comes with p = 1 only (refused on the host otherwise)
        const float d = s - p.gt[((size_t)(b * p.gh + i) * p.P + py) * Wimg + (size_t)j * p.P + px];
        lsum += (double)fabsf(d);
        const h16_t gb = f2o<BF>(d > 0.f ? ds : (d < 0.f ? -ds : 0.f));
        p.g[(size_t)m * p.ldg + n] = gb;
        csum += o2f<BF>(gb);
        if (p.s_tap) p.s_tap[(size_t)m * PP + n] = s;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + fq * 4 + r;
        if (m < M) p.g[(size_t)m * p.ldg + n] = 0;
      }
    }
    csum += __shfl_xor(csum, 16, 64);
    csum += __shfl_xor(csum, 32, 64);
    if (fq == 0) red[wave][n] = csum;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
  if (lane == 0) lred[wave] = lsum;
  __syncthreads();
  if (p.colsum_part && threadIdx.x < HF_NP)
    p.colsum_part[(size_t)blockIdx.x * HF_NP + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
}

// loss = (accumulate ? loss : 0) + scale * (the partials in a fixed order: lane l takes l, l + 64, ..., then the butterfly)
__global__ __launch_bounds__(64) void hf_loss_finish_kernel(const double* part, int n, double scale, int accumulate, double* loss) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) *loss = (accumulate ? *loss : 0.0) + scale * s;
}

// out (cols, ldo) = src (rows, lds)^T, zero in the padding columns [rows, ldo): the head's WbT (C, HF_NP) from Wb (PP, ldw), and the square
// weights of the tail's input gradients (tailfit.hip)
__global__ void hf_transpose_kernel(const h16_t* src, int lds, int rows, int cols, h16_t* out, int ldo) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= cols * ldo) return;
  const int c = idx / ldo, n = idx - c * ldo;
  out[idx] = n < rows ? src[(size_t)n * lds + c] : (h16_t)0;
}

// ---- dpre = (g WbT^T) * (A > 0 ? 1 : 0.01): 64 rows x 64 columns per workgroup ----
template <bool BF> __global__ __launch_bounds__(256) void head_da_kernel(const h16_t* g, int ldg, const h16_t* WbT, const h16_t* A, int lda,
                                                                        h16_t* dpre, int ldd, int M, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * HF_ROWS + wave * 16, c0 = blockIdx.y * 64;
  f32x4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int ma = m0 + fr;
  const h16_t* grow = g + (size_t)(ma < M ? ma : 0) * ldg + 8 * fq;
#pragma unroll
  for (int k0 = 0; k0 < HF_NP; k0 += 32) {
    const h16x8_t a = frag_load(grow + k0, ma < M);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = c0 + t * 16 + fr;  // C is a multiple of 64: always a real column
      const h16x8_t b = frag_load(WbT + (size_t)c * HF_NP + k0 + 8 * fq, true);
      acc[t] = mfma_16x16x32<BF>(a, b, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = c0 + t * 16 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + fq * 4 + r;
      if (m >= M) continue;
      const h16_t ab = A[(size_t)m * lda + c];
      const bool pos = !(ab & 0x8000) && (ab & 0x7FFF);  // the stored activation has the sign of its pre-activation; 0 takes the 0.01 side
      dpre[(size_t)m * ldd + c] = f2o<BF>(pos ? acc[t][r] : 0.01f * acc[t][r]);
    }
  }
}

// ---- gemm_tn: one (64 n, 64 k) tile of one row chunk per workgroup ----
__device__ __forceinline__ h16x8_t tile_chunk_load(const h16_t* base, int ld, int m, int m_end, int c, int ncols) {
  h16x8_t v = {};
  if (m >= m_end || c >= ncols) return v;
  const h16_t* src = base + (size_t)m * ld + c;
  if (c + 8 <= ncols) return *reinterpret_cast<const h16x8_t*>(src);
  short8_t s = {};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (c + e < ncols) s[e] = (short)src[e];
  return __builtin_bit_cast(h16x8_t, s);
}

template <bool BF> __global__ __launch_bounds__(256) void gemm_tn_kernel(CsGemmTn p, float* part, float* cs_part) {
  __shared__ __attribute__((aligned(16))) h16_t Gs[32 * HF_LROW];
  __shared__ __attribute__((aligned(16))) h16_t Xs[32 * HF_LROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64, chunk = blockIdx.z;
  const int mb = chunk * HF_CHUNK, me = min(p.M, mb + HF_CHUNK);
  const int srow = threadIdx.x >> 3, sch = (threadIdx.x & 7) * 8;  // staging: one 16-byte piece of each tile per thread
  // transposed reads: lane 4q + j of a 16-lane group names row q, columns 4j .. 4j + 3 of a 4 x 16 block and receives the block's column
  // (lane & 15) -- the MFMA's k index runs over the tile's rows 8 fq .. 8 fq + 7
  const int toff = (8 * fq + (fr >> 2)) * HF_LROW + (fr & 3) * 4;
  f32x4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float csum = 0.f;
  const bool want_cs = cs_part != nullptr && blockIdx.x == 0;
  for (int ms = mb; ms < me; ms += 32) {
    const h16x8_t gv = tile_chunk_load(p.G, p.ldg, ms + srow, me, n0 + sch, p.N);
    const h16x8_t xv = tile_chunk_load(p.X, p.ldx, ms + srow, me, k0 + sch, p.K);
    __syncthreads();  // the previous step's reads are done
    *reinterpret_cast<h16x8_t*>(&Gs[srow * HF_LROW + sch]) = gv;
    *reinterpret_cast<h16x8_t*>(&Xs[srow * HF_LROW + sch]) = xv;
    __syncthreads();
    typedef __attribute__((address_space(3))) short4_t* lds4_t;
    const short4_t alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(Gs + toff + wave * 16));
    const short4_t ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(Gs + toff + 4 * HF_LROW + wave * 16));
    const h16x8_t a = __builtin_bit_cast(h16x8_t, __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const short4_t blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(Xs + toff + t * 16));
      const short4_t bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(Xs + toff + 4 * HF_LROW + t * 16));
      const h16x8_t b = __builtin_bit_cast(h16x8_t, __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[t] = mfma_16x16x32<BF>(a, b, acc[t]);
    }
    if (want_cs && threadIdx.x < 64) {
#pragma unroll 8
      for (int r = 0; r < 32; ++r) csum += o2f<BF>(Gs[r * HF_LROW + threadIdx.x]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t * 16 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wave * 16 + fq * 4 + r;
      if (n < p.N && k < p.K) part[((size_t)chunk * p.N + n) * p.K + k] = acc[t][r];
    }
  }
  if (want_cs && threadIdx.x < 64 && n0 + (int)threadIdx.x < p.N) cs_part[(size_t)chunk * p.N + n0 + threadIdx.x] = csum;
}

// out = (accumulate ? out : 0) + scale * (the chunks' partials in chunk order); behind the N * K products, the N column sums
__global__ void gemm_tn_reduce_kernel(CsGemmTn p, const float* part, const float* cs_part, int chunks) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nk = (size_t)p.N * p.K;
  if (idx < nk) {
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * nk + idx];
    const int n = (int)(idx / p.K), k = (int)(idx - (size_t)n * p.K);
    float* o = p.out + (size_t)n * p.ldo + k;
    *o = (p.accumulate ? *o : 0.f) + p.scale * s;
  } else if (p.colsum && idx < nk + p.N) {
    const int n = (int)(idx - nk);
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += cs_part[(size_t)c * p.N + n];
    p.colsum[n] = (p.accumulate ? p.colsum[n] : 0.f) + p.scale * s;
  }
}

// ---- AdamW (torch.optim.AdamW, single tensor, amsgrad off); c1 = 1 - beta1^t and rc2 = 1 / sqrt(1 - beta2^t) come from the host in fp64 ----
__global__ void adamw_kernel(float* p, float* m, float* v, const float* g, long long n, float lr, float beta1, float beta2, float eps, float wd,
                             float c1, float rc2, h16_t* p16, int bf) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  float pi = p[i] * (1.0f - lr * wd);
  const float mi = m[i] + (gi - m[i]) * (1.0f - beta1);
  const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
  const float denom = sqrtf(vi) * rc2 + eps;
  pi -= (lr / c1) * (mi / denom);
  p[i] = pi; m[i] = mi; v[i] = vi;
  if (p16) p16[i] = f2o(pi, bf);
}

}  // namespace

extern "C" {

int cs_headfit_supported(int C, int P) { return P == 14 && C >= 64 && C % 64 == 0 && C <= 4096; }

size_t cs_gemm_tn_workspace(int M, int N, int K) {
  const size_t chunks = (size_t)(M + HF_CHUNK - 1) / HF_CHUNK;
  return up256(chunks * N * K * 4) + up256(chunks * N * 4);
}

size_t cs_head_grad_z_workspace(int M) { return up256((size_t)((M + HF_ROWS - 1) / HF_ROWS) * 8); }

hipError_t cs_head_grad_z_launch(const CsHeadGradZ* p, void* ws, int bf, hipStream_t st) {
  const int M = p->B * p->gh * p->gw, nwg = (M + HF_ROWS - 1) / HF_ROWS;
  double* part = static_cast<double*>(ws);
  if (bf) head_grad_z_kernel<true><<<nwg, 256, 0, st>>>(*p, part);
  else head_grad_z_kernel<false><<<nwg, 256, 0, st>>>(*p, part);
  hf_loss_finish_kernel<<<1, 64, 0, st>>>(part, nwg, p->loss_scale, p->loss_accumulate, p->loss);
  return hipGetLastError();
}

hipError_t cs_gemm_tn_launch(const CsGemmTn* p, void* ws, int bf, hipStream_t st) {
  const int chunks = (p->M + HF_CHUNK - 1) / HF_CHUNK;
  float* part = static_cast<float*>(ws);
  float* cs_part = reinterpret_cast<float*>(static_cast<char*>(ws) + up256((size_t)chunks * p->N * p->K * 4));
  const dim3 grid((p->K + 63) / 64, (p->N + 63) / 64, chunks);
  if (bf) gemm_tn_kernel<true><<<grid, 256, 0, st>>>(*p, part, p->colsum ? cs_part : nullptr);
  else gemm_tn_kernel<false><<<grid, 256, 0, st>>>(*p, part, p->colsum ? cs_part : nullptr);
  const size_t total = (size_t)p->N * p->K + (p->colsum ? p->N : 0);
  gemm_tn_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(*p, part, cs_part, chunks);
  return hipGetLastError();
}

// the workspace of one whole backward: head_carve (fit_shared.h), which the launch below takes its pointers from
size_t cs_head_backward_workspace(int M, int C) { return head_carve(nullptr, M, C).end; }

hipError_t cs_transpose16_launch(const h16_t* src, int lds, int rows, int cols, h16_t* out, int ldo, hipStream_t st) {
  hf_transpose_kernel<<<(cols * ldo + 255) / 256, 256, 0, st>>>(src, lds, rows, cols, out, ldo);
  return hipGetLastError();
}

hipError_t cs_head_backward_launch(const CsHeadBackward* q, void* ws, int bf, hipStream_t st) {
  const int M = q->B * q->gh * q->gw, C = q->C, PP = q->P * q->P;
  const HeadWs k = head_carve(ws, M, C);
  h16_t *g = k.g, *dpre = k.dpre, *WbT = k.WbT;
  void *zws = k.zws, *tws = k.tws;
  CsHeadGradZ z{};
  z.A = q->A; z.lda = q->lda; z.Wb = q->Wb; z.ldw = q->ldw; z.bb = q->bb; z.gt = q->gt; z.B = q->B; z.gh = q->gh; z.gw = q->gw; z.P = q->P; z.C = C;
  z.act = q->act; z.powp = q->powp; z.g = g; z.ldg = HF_NP; z.loss = q->loss; z.loss_scale = q->inv_count; z.loss_accumulate = q->accumulate;
  hipError_t e = cs_head_grad_z_launch(&z, zws, bf, st);
  if (e != hipSuccess) return e;
  hf_transpose_kernel<<<(C * HF_NP + 255) / 256, 256, 0, st>>>(q->Wb, q->ldw, PP, C, WbT, HF_NP);
  const dim3 grid((M + HF_ROWS - 1) / HF_ROWS, C / 64);
  if (bf) head_da_kernel<true><<<grid, 256, 0, st>>>(g, HF_NP, WbT, q->A, q->lda, dpre, C, M, C);
  else head_da_kernel<false><<<grid, 256, 0, st>>>(g, HF_NP, WbT, q->A, q->lda, dpre, C, M, C);
  CsGemmTn t{};
  t.G = g; t.ldg = HF_NP; t.X = q->A; t.ldx = q->lda; t.M = M; t.N = PP; t.K = C; t.scale = (float)q->inv_count; t.accumulate = q->accumulate;
  t.out = q->dWb; t.ldo = C; t.colsum = q->dbb;
  e = cs_gemm_tn_launch(&t, tws, bf, st);  // dWb, dbb
  if (e != hipSuccess) return e;
  t.G = dpre; t.ldg = C; t.X = q->X; t.ldx = q->ldx; t.N = C; t.out = q->dWa; t.colsum = q->dba;
  return cs_gemm_tn_launch(&t, tws, bf, st);  // dWa, dba (stream order: the partials of dWb have been reduced)
}

hipError_t cs_adamw_launch(float* p, float* m, float* v, const float* g, long long n, float lr, float beta1, float beta2, float eps, float wd,
                           int step, h16_t* p16, int bf, hipStream_t st) {
  const double c1 = 1.0 - std::pow((double)beta1, (double)step), c2 = 1.0 - std::pow((double)beta2, (double)step);
  adamw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p, m, v, g, n, lr, beta1, beta2, eps, wd, (float)c1, (float)(1.0 / std::sqrt(c2)), p16, bf);
  return hipGetLastError();
}

}
