// Score pooling on the device (gfx950): per image of a batch of H x W maps of 16-bit codes the exact sum, the
// order statistics s[(q (n - 1)) / 1000], the sums of the k = max(1, (q n) / 1000) smallest codes, and the S x S window of the smallest sum
// (include/crossscore_hip.h states the definition).  The maps are uint16 samples or fp32 scores, whose codes are cs_score_code (cs_common.h,
// what score_gray16_kernel stores).  Integers throughout: an image's words do not depend on its place in the batch or on the order of
// workgroups and atomics.
//
// Order statistics and tails are a two-level radix select over the code's high 12 and low 4 bits; every step is a launch of its own, so the
// launch boundary is the only synchronisation between workgroups:
//   pool_coarse_kernel   a workgroup owns a band of rows and counts it into an LDS histogram of the 4096 coarse bins: per bin the number of
//                        codes and the sum of their low 4 bits (both u32: n <= 2^24, 15 n < 2^32; the all-equal map fills one word with n).
//                        Non-zero bins are flushed to the image's (2, 4096) table with vector atomics: at most 8192 per ~16K pixels.
//   pool_select_kernel   one workgroup per image walks that table: the image's sum, and per requested rank (Q quantile indices, Q tail
//                        indices k - 1) the coarse bin holding it, the rank inside the bin and the sum of all codes in lower bins.
//   pool_fine_kernel     rereads the image and counts the low 4 bits of the codes that fall into one of the <= 2Q chosen bins (an LDS
//                        byte table maps coarse bin -> slot), flushed to the image's (32, 16) table.
//   pool_resolve_kernel  one thread per rank walks its slot's 16 counters: the quantile's code, or the tail's sum.  It also decodes the
//                        window key.
// Worst window: separable sums in u32.  window_rows_kernel forms per row the sums of S neighbouring codes (< 2^24) from a wrapping u32 prefix
// sum of the row in LDS; window_cols_kernel slides S of those down each column (window sums < 2^32: 65535 x 255^2) and keeps the smallest
// key  sum << 24 | y << 12 | x  (H, W <= 4096), one 64-bit atomicMin per workgroup: ties go to the smallest y, then the smallest x.
#include "cs_common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kCoarse = 4096, kSlots = 32, kFine = 16;  // coarse bins (high 12 bits), ranks per image (2 x 16), codes per coarse bin
constexpr int kBandPixels = 16384;                      // pixels a workgroup of the two counting kernels owns, about
constexpr int kRowsPerBlock = 4, kColBand = 16;         // window_rows_kernel: rows per workgroup; window_cols_kernel: output rows per thread

struct PoolRanks { uint32_t r[kSlots]; };  // [0, Q): quantile indices; [Q, 2Q): k - 1, the index of the last code a tail takes
struct PoolSel { uint32_t bin, inside; unsigned long long below; };  // coarse bin of a rank, the rank inside it, the sum of all codes in lower bins

template <typename T> __device__ __forceinline__ uint32_t code_at(const T* p, int signed_range);
template <> __device__ __forceinline__ uint32_t code_at<uint16_t>(const uint16_t* p, int) { return *p; }
template <> __device__ __forceinline__ uint32_t code_at<float>(const float* p, int signed_range) { return cs_score_code(*p, signed_range); }

template <typename T>
__global__ __launch_bounds__(kThreads) void pool_coarse_kernel(const T* __restrict__ map, int H, int W, int row_elems, long long image_stride,
                                                               int rows_per, int signed_range, uint32_t* __restrict__ cnt_tab,
                                                               uint32_t* __restrict__ low_tab) {
  __shared__ uint32_t cnt[kCoarse], low[kCoarse];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  for (int i = tid; i < kCoarse; i += kThreads) cnt[i] = low[i] = 0;
  __syncthreads();
  const int y0 = blockIdx.x * rows_per, y1 = min(H, y0 + rows_per);
  for (int y = y0 + wave; y < y1; y += kWaves) {
    const T* row = map + (long long)b * image_stride + (long long)y * row_elems;
    for (int x = lane; x < W; x += 64) {
      const uint32_t c = code_at<T>(row + x, signed_range);
      atomicAdd(&cnt[c >> 4], 1u);
      atomicAdd(&low[c >> 4], c & 15u);
    }
  }
  __syncthreads();
  for (int i = tid; i < kCoarse; i += kThreads) {
    const uint32_t n = cnt[i], l = low[i];
    if (n) atomicAdd(cnt_tab + (size_t)b * kCoarse + i, n);
    if (l) atomicAdd(low_tab + (size_t)b * kCoarse + i, l);
  }
}

// thread t owns the coarse bins [16 t, 16 t + 16)
__global__ __launch_bounds__(kThreads) void pool_select_kernel(const uint32_t* __restrict__ cnt_tab, const uint32_t* __restrict__ low_tab,
                                                               PoolRanks ranks, int nr, PoolSel* __restrict__ sel,
                                                               unsigned long long* __restrict__ sum_out) {
  __shared__ uint32_t pc[kThreads];
  __shared__ unsigned long long ps[kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  const uint4* cp = reinterpret_cast<const uint4*>(cnt_tab + (size_t)b * kCoarse + t * 16);
  const uint4* lp = reinterpret_cast<const uint4*>(low_tab + (size_t)b * kCoarse + t * 16);
  uint32_t c[16];
  unsigned long long s[16];  // the sum of the codes of each bin: count x (bin << 4) + the sum of the low bits
  uint32_t lc = 0;
  unsigned long long ls = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const uint4 cv = cp[v], lv = lp[v];
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * v + j;
      c[i] = cw[j];
      s[i] = (unsigned long long)cw[j] * (unsigned long long)((uint32_t)(t * 16 + i) << 4) + lw[j];
      lc += c[i];
      ls += s[i];
    }
  }
  pc[t] = lc;
  ps[t] = ls;
  __syncthreads();
  uint32_t bc = 0;  // codes and their sum in the bins below this thread's
  unsigned long long bs = 0;
  for (int i = 0; i < t; ++i) {
    bc += pc[i];
    bs += ps[i];
  }
  if (t == kThreads - 1) sum_out[b] = bs + ls;
  for (int r = 0; r < nr; ++r) {
    const uint32_t rank = ranks.r[r];
    if (rank < bc || rank - bc >= lc) continue;  // exactly one thread holds a rank below n
    uint32_t cum = bc;
    unsigned long long below = bs;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (!found) {
        if (rank - cum < c[i]) {
          PoolSel e;
          e.bin = (uint32_t)(t * 16 + i);
          e.inside = rank - cum;
          e.below = below;
          sel[(size_t)b * kSlots + r] = e;
          found = true;
        } else {
          cum += c[i];
          below += s[i];
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pool_fine_kernel(const T* __restrict__ map, int H, int W, int row_elems, long long image_stride,
                                                             int rows_per, int signed_range, const PoolSel* __restrict__ sel, int nr,
                                                             uint32_t* __restrict__ fine_tab) {
  __shared__ uint32_t lut_words[kCoarse / 4];  // per coarse bin the slot that counts it, 0xFF for none
  __shared__ uint32_t fine[kSlots * kFine];
  uint8_t* lut = reinterpret_cast<uint8_t*>(lut_words);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  for (int i = tid; i < kCoarse / 4; i += kThreads) lut_words[i] = 0xFFFFFFFFu;
  for (int i = tid; i < kSlots * kFine; i += kThreads) fine[i] = 0;
  __syncthreads();
  if (tid == 0)
    for (int r = 0; r < nr; ++r) {  // ranks that share a bin share the slot of the first of them
      const uint32_t bin = sel[(size_t)b * kSlots + r].bin & (kCoarse - 1);
      if (lut[bin] == 0xFF) lut[bin] = (uint8_t)r;
    }
  __syncthreads();
  const int y0 = blockIdx.x * rows_per, y1 = min(H, y0 + rows_per);
  for (int y = y0 + wave; y < y1; y += kWaves) {
    const T* row = map + (long long)b * image_stride + (long long)y * row_elems;
    for (int x = lane; x < W; x += 64) {
      const uint32_t c = code_at<T>(row + x, signed_range);
      const uint32_t slot = lut[c >> 4];
      if (slot != 0xFF) atomicAdd(&fine[slot * kFine + (c & 15u)], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < kSlots * kFine; i += kThreads)
    if (fine[i]) atomicAdd(fine_tab + (size_t)b * kSlots * kFine + i, fine[i]);
}

__global__ __launch_bounds__(64) void pool_resolve_kernel(const PoolSel* __restrict__ sel, const uint32_t* __restrict__ fine_tab, int Q,
                                                          uint32_t* __restrict__ quant, unsigned long long* __restrict__ tail,
                                                          const unsigned long long* __restrict__ key, unsigned long long* __restrict__ window) {
  const int r = threadIdx.x, b = blockIdx.x;
  if (r < 2 * Q) {
    const PoolSel e = sel[(size_t)b * kSlots + r];
    int slot = r;
    for (int k = r - 1; k >= 0; --k)
      if (sel[(size_t)b * kSlots + k].bin == e.bin) slot = k;
    const uint32_t* f = fine_tab + ((size_t)b * kSlots + slot) * kFine;
    if (r < Q) {
      uint32_t cum = 0, code = e.bin << 4;
      bool found = false;
      for (int i = 0; i < kFine; ++i) {
        cum += f[i];
        if (!found && e.inside < cum) {
          code = (e.bin << 4) | (uint32_t)i;
          found = true;
        }
      }
      quant[(size_t)b * Q + r] = code;
    } else {
      uint32_t take = e.inside + 1;
      unsigned long long t = e.below;
      for (int i = 0; i < kFine; ++i) {
        const uint32_t m = min(f[i], take);
        t += (unsigned long long)m * (unsigned long long)((e.bin << 4) | (uint32_t)i);
        take -= m;
      }
      tail[(size_t)b * Q + (r - Q)] = t;
    }
  }
  if (r == 63 && window) {
    const unsigned long long k = key[b];
    window[3 * (size_t)b] = k >> 24;
    window[3 * (size_t)b + 1] = (k >> 12) & 4095u;
    window[3 * (size_t)b + 2] = k & 4095u;
  }
}

// hs (B, H, nx), nx = W - S + 1: hs[y][x] = the sum of the S codes of row y from column x on
template <typename T>
__global__ __launch_bounds__(kThreads) void window_rows_kernel(const T* __restrict__ map, int H, int W, int row_elems, long long image_stride,
                                                               int signed_range, int S, uint32_t* __restrict__ hs) {
  __shared__ uint32_t row[4096];
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  const int nx = W - S + 1, E = (W + kThreads - 1) / kThreads;
  const int x0 = tid * E, x1 = min(W, x0 + E);  // this thread's share of the prefix sum (empty behind the row's end)
  for (int yy = 0; yy < kRowsPerBlock; ++yy) {
    const int y = blockIdx.x * kRowsPerBlock + yy;
    if (y >= H) break;  // (the same for the whole workgroup)
    const T* src = map + (long long)b * image_stride + (long long)y * row_elems;
    for (int x = tid; x < W; x += kThreads) row[x] = code_at<T>(src + x, signed_range);
    __syncthreads();
    uint32_t s = 0;
    for (int x = x0; x < x1; ++x) s += row[x];
    uint32_t inc = s;  // inclusive scan over the wave; sums wrap in 32 bits, differences of S <= 255 neighbours do not
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - s;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    for (int x = x0; x < x1; ++x) {
      run += row[x];
      row[x] = run;
    }
    __syncthreads();
    uint32_t* out = hs + ((size_t)b * H + y) * nx;
    for (int x = tid; x < nx; x += kThreads) out[x] = row[x + S - 1] - (x ? row[x - 1] : 0u);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void window_cols_kernel(const uint32_t* __restrict__ hs, int H, int nx, int S,
                                                               unsigned long long* __restrict__ key) {
  __shared__ unsigned long long red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
  const int x = blockIdx.x * kThreads + tid, ny = H - S + 1;
  const int y0 = blockIdx.y * kColBand, y1 = min(ny, y0 + kColBand);
  unsigned long long best = ~0ull;
  if (x < nx && y0 < y1) {
    const uint32_t* p = hs + (size_t)b * H * nx + x;
    uint32_t s = 0;
#pragma unroll 8
    for (int i = 0; i < S; ++i) s += p[(size_t)(y0 + i) * nx];
    for (int y = y0;;) {
      const unsigned long long k = ((unsigned long long)s << 24) | ((unsigned long long)y << 12) | (unsigned long long)x;
      best = k < best ? k : best;
      if (++y >= y1) break;
      s += p[(size_t)(y + S - 1) * nx] - p[(size_t)(y - 1) * nx];
    }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long v = __shfl_xor(best, o, 64);
    best = v < best ? v : best;
  }
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) best = red[w] < best ? red[w] : best;
    if (best != ~0ull) atomicMin(key + b, best);
  }
}

// the scratch of one call: [coarse counts | coarse low sums | fine counts] (zeroed per call), the selections, the window keys, the row sums
struct Layout { size_t cnt, low, fine, zero_end, sel, key, hs, end; };
Layout layout(int B, int H, int W) {
  Layout l;
  size_t at = 0;
  l.cnt = at; at += (size_t)B * kCoarse * sizeof(uint32_t);
  l.low = at; at += (size_t)B * kCoarse * sizeof(uint32_t);
  l.fine = at; at += (size_t)B * kSlots * kFine * sizeof(uint32_t);
  l.zero_end = at;
  l.sel = at; at += (size_t)B * kSlots * sizeof(PoolSel);
  l.key = at; at += ((size_t)B * sizeof(unsigned long long) + 15) / 16 * 16;
  l.hs = at; at += (size_t)B * H * W * sizeof(uint32_t);  // (S = 1: the largest the row sums get)
  l.end = at;
  return l;
}

template <typename T>
hipError_t launch(const T* map, int B, int H, int W, int row_elems, long long image_stride, int signed_range, const uint32_t* ranks, int Q, int S,
                  uint64_t* sum, uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch, hipStream_t st) {
  const Layout l = layout(B, H, W);
  char* base = static_cast<char*>(scratch);
  uint32_t* cnt_tab = reinterpret_cast<uint32_t*>(base + l.cnt);
  uint32_t* low_tab = reinterpret_cast<uint32_t*>(base + l.low);
  uint32_t* fine_tab = reinterpret_cast<uint32_t*>(base + l.fine);
  PoolSel* sel = reinterpret_cast<PoolSel*>(base + l.sel);
  unsigned long long* key = reinterpret_cast<unsigned long long*>(base + l.key);
  uint32_t* hs = reinterpret_cast<uint32_t*>(base + l.hs);
  PoolRanks pr{};
  for (int r = 0; r < 2 * Q; ++r) pr.r[r] = ranks[r];
  hipError_t e = hipMemsetAsync(base, 0, l.zero_end, st);
  if (e != hipSuccess) return e;
  const bool win = window != nullptr && S > 0;
  if (win) {
    e = hipMemsetAsync(key, 0xFF, (size_t)B * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  const int rows_per = max(1, kBandPixels / W);
  const dim3 bands((H + rows_per - 1) / rows_per, B);
  hipLaunchKernelGGL(pool_coarse_kernel<T>, bands, dim3(kThreads), 0, st, map, H, W, row_elems, image_stride, rows_per, signed_range, cnt_tab, low_tab);
  hipLaunchKernelGGL(pool_select_kernel, dim3(B), dim3(kThreads), 0, st, cnt_tab, low_tab, pr, 2 * Q, sel,
                     reinterpret_cast<unsigned long long*>(sum));
  hipLaunchKernelGGL(pool_fine_kernel<T>, bands, dim3(kThreads), 0, st, map, H, W, row_elems, image_stride, rows_per, signed_range, sel, 2 * Q, fine_tab);
  if (win) {
    const int nx = W - S + 1, ny = H - S + 1;
    hipLaunchKernelGGL(window_rows_kernel<T>, dim3((H + kRowsPerBlock - 1) / kRowsPerBlock, B), dim3(kThreads), 0, st, map, H, W, row_elems,
                       image_stride, signed_range, S, hs);
    hipLaunchKernelGGL(window_cols_kernel, dim3((nx + kThreads - 1) / kThreads, (ny + kColBand - 1) / kColBand, B), dim3(kThreads), 0, st, hs, H, nx,
                       S, key);
  }
  hipLaunchKernelGGL(pool_resolve_kernel, dim3(B), dim3(64), 0, st, sel, fine_tab, Q, quant, reinterpret_cast<unsigned long long*>(tail), key,
                     win ? reinterpret_cast<unsigned long long*>(window) : nullptr);
  return hipGetLastError();
}

}  // namespace

extern "C" size_t cs_scorepool_workspace(int B, int H, int W) { return layout(B, H, W).end; }

// arguments are checked by the caller (ops.hip); ranks: 2Q host words, the quantile indices and behind them k - 1 of every tail
extern "C" hipError_t cs_scorepool_launch(const void* map, int is_f32, int B, int H, int W, int row_elems, long long image_stride,
                                          int signed_range, const uint32_t* ranks, int Q, int S, uint64_t* sum, uint32_t* quant, uint64_t* tail,
                                          uint64_t* window, void* scratch, hipStream_t st) {
  if (is_f32)
    return launch(static_cast<const float*>(map), B, H, W, row_elems, image_stride, signed_range, ranks, Q, S, sum, quant, tail, window, scratch, st);
  return launch(static_cast<const uint16_t*>(map), B, H, W, row_elems, image_stride, 0, ranks, Q, S, sum, quant, tail, window, scratch, st);
}
