// Reference selection by DINOv2 similarity: pooled token descriptors, their centre over a bank, unit vectors, similarities,
// the N best bank entries per query and the gather of their token blocks.  Plain vector code: fp32 arithmetic, fixed summation orders that
// depend on the problem's sizes only -- never on how many images a launch holds or where an image sits in it -- and no atomics.
#include "cs_common.h"

namespace {

constexpr int DESC_COLS = 64;    // columns of one descriptor workgroup: 8 lanes x 8 columns (one 16-byte load each)
constexpr int DESC_ROWS = 32;    // row lanes of it: lane r sums the rows r, r + 32, r + 64, ... in that order
constexpr int CENTRE_ROWS = 4;   // row lanes of the centre kernel (one wave each)
constexpr int TOPN_THREADS = 256;
constexpr int GATHER_VECS = 4;   // 16-byte vectors per thread of the gather: a workgroup copies 256 x 4 x 16 = 16 KiB of a slot

// m[img][c] = (1 / Np) sum_p t[img][p][c].  Workgroup (slab, img): 64 columns of one image.  Thread (r, g): row lane r of 32, columns
// 8 g .. 8 g + 7 of the slab.  Order: each row lane adds its rows in ascending order; the 32 partial sums are then added as a binary tree over
// the row lanes (16, 8, 4, 2, 1 apart) in LDS.  The image's index enters the addresses only.
template <bool BF>
__global__ __launch_bounds__(256) void token_descriptor_kernel(const h16_t* __restrict__ tok, int Np, int C, float* __restrict__ mean) {
  __shared__ float part[DESC_ROWS][DESC_COLS + 4];
  const int g = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int c0 = blockIdx.x * DESC_COLS + g * 8;
  const h16_t* src = tok + (size_t)blockIdx.y * Np * C + c0;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = r; p < Np; p += DESC_ROWS) {
    const short8_t v = *reinterpret_cast<const short8_t*>(src + (size_t)p * C);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += o2f<BF>((h16_t)v[k]);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[r][g * 8 + k] = acc[k];
  __syncthreads();
#pragma unroll
  for (int s = DESC_ROWS / 2; s >= 1; s >>= 1) {
    if (r < s) {
#pragma unroll
      for (int k = 0; k < 8; ++k) part[r][g * 8 + k] += part[r + s][g * 8 + k];
    }
    __syncthreads();
  }
  if (threadIdx.x < DESC_COLS) mean[(size_t)blockIdx.y * C + blockIdx.x * DESC_COLS + threadIdx.x] = part[0][threadIdx.x] / (float)Np;
}

// centre[c] = (1 / R) sum_r m[r][c]: a workgroup per 64 columns, wave w adds the rows w, w + 4, ... in ascending order, then (p0 + p1) + (p2 + p3)
__device__ __forceinline__ void centre_columns(const float* __restrict__ mean, int R, int C, float* __restrict__ centre) {
  __shared__ float part[CENTRE_ROWS][64];
  const int col = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + col;
  float acc = 0.f;
#pragma unroll 8
  for (int r = w; r < R; r += CENTRE_ROWS) acc += mean[(size_t)r * C + c];
  part[w][col] = acc;
  __syncthreads();
  if (w == 0) centre[c] = ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) / (float)R;
}

// Which rows: group g of a grouped bank is the rows offsets[g] .. offsets[g + 1] - 1 of its R rows; without offsets (null) the
// bank is one group of all R rows.  The branch is uniform over the launch.  The host has checked the offsets; the device still clamps what it
// reads from them, so that no address leaves [0, R) whatever the array holds.
__device__ __forceinline__ void group_rows(const int* __restrict__ offsets, int g, int R, int& lo, int& n) {
  if (!offsets) { lo = 0; n = R; return; }
  lo = min(max(offsets[g], 0), R);
  n = min(max(offsets[g + 1], lo), R) - lo;
}

// centre[g] = the centre of group g's rows alone, in the order above: workgroup (64 columns, g).  The group's place enters the addresses only.
__global__ __launch_bounds__(256) void centre_kernel(const float* __restrict__ mean, const int* __restrict__ offsets, int R, int C,
                                                     float* __restrict__ centre) {
  int lo, n;
  group_rows(offsets, blockIdx.y, R, lo, n);
  centre_columns(mean + (size_t)lo * C, n, C, centre + (size_t)blockIdx.y * C);
}

// unit[i] = (m[i] - centre) / max(|m[i] - centre|, 1e-12): one wave per image; a lane squares and adds its columns lane, lane + 64, ... in
// ascending order, the 64 partial sums go through the butterfly of wave_sum.  A row equal to the centre gives zeros.
__device__ __forceinline__ void unit_row(const float* __restrict__ m, const float* __restrict__ centre, int C, float* __restrict__ unit) {
  const int lane = threadIdx.x & 63;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = m[c] - centre[c];
    ss = fmaf(d, d, ss);
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  for (int c = lane; c < C; c += 64) unit[c] = (m[c] - centre[c]) * inv;
}

// the bank's units, every row against its own group's centre (G, C): one wave per row below offsets[G]; the rows behind are left alone.  A wave
// finds its row's group by bisection of the offsets (wave-uniform).  Without offsets: every row of R against the one centre.
__global__ __launch_bounds__(256) void bank_unit_kernel(const float* __restrict__ mean, const int* __restrict__ offsets, int G, int R, int C,
                                                        const float* __restrict__ centre, float* __restrict__ unit) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= (offsets ? min(offsets[G], R) : R)) return;
  int g = 0, hi = offsets ? G : 1;  // the last g with offsets[g] <= i
  while (hi - g > 1) {
    const int mid = (g + hi) >> 1;
    if (offsets[mid] <= i) g = mid; else hi = mid;
  }
  unit_row(mean + (size_t)i * C, centre + (size_t)g * C, C, unit + (size_t)i * C);
}

// What the host resolves per query of a grouped call: its group's first row, its rows and its centre (SelTriple of cs_common.h).  Without
// triples (null, uniform over the launch) every query has the whole bank and the one centre.
__device__ __forceinline__ void query_slice(const CsSelTriple* __restrict__ trip, int b, int R, int G, int& lo, int& n, int& g) {
  if (!trip) { lo = 0; n = R; g = 0; return; }
  const CsSelTriple t = trip[b];
  lo = min(max(t.start, 0), R);
  n = min(max(t.len, 0), R - lo);
  g = min(max(t.centre, 0), G - 1);
}

// the queries' units, each against the centre of its own group
__global__ __launch_bounds__(256) void query_unit_kernel(const float* __restrict__ mean, int B, int C, const CsSelTriple* __restrict__ trip, int R,
                                                         int G, const float* __restrict__ centre, float* __restrict__ unit) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int lo, n, g;
  query_slice(trip, b, R, G, lo, n, g);
  unit_row(mean + (size_t)b * C, centre + (size_t)g * C, C, unit + (size_t)b * C);
}

// sim[b][r] = sum_c q[b][c] e[r][c]: one wave per (b, r) pair; a lane takes the float4 groups lane, lane + 64, ... in ascending order (four fmas
// each, x y z w), then wave_sum.  r and b enter the addresses only, so two equal bank rows give equal bits.
__device__ __forceinline__ float wave_dot(const float* __restrict__ q, const float* __restrict__ e, int C) {
  const int lane = threadIdx.x & 63;
  const float4* qa = reinterpret_cast<const float4*>(q);
  const float4* ea = reinterpret_cast<const float4*>(e);
  float acc = 0.f;
  for (int c = lane; c < C / 4; c += 64) {
    const float4 x = qa[c], y = ea[c];
    acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
  }
  return wave_sum(acc);
}

// sim[b][j], j = 0 .. S - 1: query b against row j of its own slice of the bank; the columns behind the slice become a quiet NaN
__global__ __launch_bounds__(256) void similarity_kernel(const float* __restrict__ q, const float* __restrict__ bank, int R, int G, int C,
                                                         const CsSelTriple* __restrict__ trip, int S, float* __restrict__ sim) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (j >= S) return;
  int lo, n, g;
  query_slice(trip, b, R, G, lo, n, g);
  const float acc = j < n ? wave_dot(q + (size_t)b * C, bank + (size_t)(lo + j) * C, C) : __int_as_float(0x7fc00000);
  if ((threadIdx.x & 63) == 0) sim[(size_t)b * S + j] = acc;
}

// the order of the selection: larger similarity first, the lower index among equals
__device__ __forceinline__ bool sel_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// index[n], n = 0 .. N - 1: the N first of the R similarities s in the order above, entry ex left out, each reported as its place + base.  One
// workgroup; round n takes the first entry that comes strictly behind round n - 1's pick, so nothing is marked and s stays as the caller sees it.
// Fewer than N candidates (similarities that are NaN never qualify) leave -1 in the remaining places.
__device__ __forceinline__ void topn_row(const float* __restrict__ s, int R, int ex, int N, int base, int* __restrict__ index) {
  __shared__ float ws[TOPN_THREADS / 64];
  __shared__ int wi[TOPN_THREADS / 64];
  __shared__ float pick_s;
  __shared__ int pick_i;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float prev_s = 0.f;
  int prev_i = -1;  // -1: no pick yet, every entry qualifies
  for (int n = 0; n < N; ++n) {
    float bs = 0.f;
    int bi = -1;
    for (int r = threadIdx.x; r < R; r += TOPN_THREADS) {
      const float v = s[r];
      if (r == ex || v != v) continue;
      if (prev_i >= 0 && !sel_before(prev_s, prev_i, v, r)) continue;
      if (bi < 0 || sel_before(v, r, bs, bi)) { bs = v; bi = r; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi >= 0 && (bi < 0 || sel_before(os, oi, bs, bi))) { bs = os; bi = oi; }
    }
    if (lane == 0) { ws[w] = bs; wi[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < TOPN_THREADS / 64; ++k)
        if (wi[k] >= 0 && (bi < 0 || sel_before(ws[k], wi[k], bs, bi))) { bs = ws[k]; bi = wi[k]; }
      pick_s = bs; pick_i = bi;
      index[n] = bi < 0 ? -1 : bi + base;
    }
    __syncthreads();
    prev_s = pick_s; prev_i = pick_i;
    if (prev_i < 0) {  // (uniform over the workgroup) nothing left: the remaining places say so
      if (threadIdx.x == 0) for (int k = n + 1; k < N; ++k) index[k] = -1;
      return;
    }
    __syncthreads();  // pick_s / pick_i are rewritten by the next round
  }
}

// one workgroup per query over its slice of the bank: sim is (B, S), the picks are reported as bank rows, exclude[b] is a bank row (one outside
// the slice matches no place of it)
__global__ __launch_bounds__(TOPN_THREADS) void topn_kernel(const float* __restrict__ sim, int S, int R, int G, const CsSelTriple* __restrict__ trip,
                                                            const int* __restrict__ exclude, int N, int* __restrict__ index) {
  const int b = blockIdx.x;
  int lo, n, g;
  query_slice(trip, b, R, G, lo, n, g);
  const int ex = exclude ? exclude[b] : -1;
  topn_row(sim + (size_t)b * S, min(n, S), ex >= lo ? ex - lo : -1, N, lo, index + (size_t)b * N);
}

// out[slot] = bank[index[slot]] as 16-byte vectors, `vecs` of them per slot; an index outside [0, R) reads bank row `blank` when that lies in
// [0, R), else nothing and its slot becomes zeros
__global__ __launch_bounds__(256) void gather_tokens_kernel(const uint4* __restrict__ bank, int R, size_t vecs, const int* __restrict__ index,
                                                            int blank, uint4* __restrict__ out) {
  const int slot = blockIdx.y;
  int src = index[slot];
  if (src < 0 || src >= R) src = blank;
  const bool ok = src >= 0 && src < R;
  const uint4* from = bank + (ok ? (size_t)src * vecs : 0);
  uint4* to = out + (size_t)slot * vecs;
  const size_t v0 = (size_t)blockIdx.x * (256 * GATHER_VECS) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < GATHER_VECS; ++k) {
    const size_t v = v0 + (size_t)k * 256;
    if (v < vecs) to[v] = ok ? from[v] : uint4{0u, 0u, 0u, 0u};
  }
}

}  // namespace

extern "C" {

// tok (I, Np, C) 16-bit, C a multiple of 64 -> mean (I, C) fp32
hipError_t cs_token_descriptors_launch(const h16_t* tok, int I, int Np, int C, int bf, float* mean, hipStream_t st) {
  const dim3 grid((unsigned)(C / DESC_COLS), (unsigned)I);
  if (bf) hipLaunchKernelGGL(token_descriptor_kernel<true>, grid, dim3(256), 0, st, tok, Np, C, mean);
  else hipLaunchKernelGGL(token_descriptor_kernel<false>, grid, dim3(256), 0, st, tok, Np, C, mean);
  return hipGetLastError();
}

// offsets (G + 1) and trip (B) are DEVICE copies of what the host resolved and checked, G <= 65535, G >= 1; null for a plain bank: one group of
// all R rows (G = 1, S = R)
hipError_t cs_centre_launch(const float* mean, const int32_t* offsets, int G, int R, int C, float* centre, hipStream_t st) {
  hipLaunchKernelGGL(centre_kernel, dim3((unsigned)(C / 64), (unsigned)G), dim3(256), 0, st, mean, offsets, R, C, centre);
  return hipGetLastError();
}

hipError_t cs_bank_unit_launch(const float* mean, const int32_t* offsets, int G, int rows, int R, int C, const float* centre, float* unit, hipStream_t st) {
  hipLaunchKernelGGL(bank_unit_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, mean, offsets, G, R, C, centre, unit);
  return hipGetLastError();
}

hipError_t cs_query_unit_launch(const float* mean, int B, int C, const CsSelTriple* trip, int R, int G, const float* centre, float* unit, hipStream_t st) {
  hipLaunchKernelGGL(query_unit_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, mean, B, C, trip, R, G, centre, unit);
  return hipGetLastError();
}

// sim (B, S) = q (B, C) x each query's slice of bank (R, C)^T: the grid is sized by the longest slice, not by the bank; C a multiple of 4, B <= 65535
hipError_t cs_similarity_launch(const float* q, int B, const float* bank, int R, int G, int C, const CsSelTriple* trip, int S, float* sim, hipStream_t st) {
  hipLaunchKernelGGL(similarity_kernel, dim3((unsigned)((S + 3) / 4), (unsigned)B), dim3(256), 0, st, q, bank, R, G, C, trip, S, sim);
  return hipGetLastError();
}

hipError_t cs_topn_launch(const float* sim, int B, int S, int R, int G, const CsSelTriple* trip, const int32_t* exclude, int N, int32_t* index, hipStream_t st) {
  hipLaunchKernelGGL(topn_kernel, dim3((unsigned)B), dim3(TOPN_THREADS), 0, st, sim, S, R, G, trip, exclude, N, index);
  return hipGetLastError();
}

// out (slots, Np, C) <- bank (R, Np, C) rows named by index (slots); Np * C a multiple of 8 (16-byte vectors), slots <= 65535
hipError_t cs_gather_tokens_launch(const h16_t* bank, int R, int Np, int C, const int32_t* index, int slots, int blank, h16_t* out, hipStream_t st) {
  const size_t vecs = (size_t)Np * C / 8;
  const size_t per_block = 256 * GATHER_VECS;
  hipLaunchKernelGGL(gather_tokens_kernel, dim3((unsigned)((vecs + per_block - 1) / per_block), (unsigned)slots), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(bank), R, vecs, index, blank, reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

}  // extern "C"
