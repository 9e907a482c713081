// Ground-truth metric maps on the device (gfx950): a render and the captured image of the same view, both uint8 HWC RGB, in; the uint16 map
// that NvsDataset reads from <iter>/metric_map/{ssim,mae}/ out (DESIGN.md section 6, row f6 holds the definition).
//
// SSIM kind (gt_ssim_kernel): one workgroup of 256 threads owns a 16 x 64 output tile plus a 5-pixel halo, 26 x 74 pixels of both images.
//   a. the bytes of that region go to LDS once, as the aligned dwords that cover each row's span (a dword that is not wholly inside the
//      image's own bytes is put together from single bytes: nothing outside the image is read)
//   b. a shift c per image and channel: the rounded integer mean of the tile's own pixels (integer sums: no order dependence)
//   c. per channel: the width pass of the five moment planes G*(a-c_a), G*(b-c_b), G*(a-c_a)^2, G*(b-c_b)^2, G*(a-c_a)(b-c_b) into LDS (26 rows
//      x 64 columns each), a barrier, the height pass out of LDS (a thread owns one column of four output rows), then the SSIM term
//   d. the mean of the three channels -> trunc((m + 1) * 32767), stored as lines of uint16 (one wave = 64 consecutive samples of a row)
//   Pixels are integers 0..255 here, not x / 255: SSIM is a ratio of second-order terms, so C1 and C2 are scaled by 255^2 instead.  A pixel
//   outside the image has value 0 and keeps its weight (zero padding), i.e. -c after the shift.
//   Why the shift: variances and the covariance do not change when a constant is taken off the pixels, the means change by that constant
//   (the 121 weights sum to 1, padded zeros included).  Without it G*(a*a) - mu_a^2 cancels catastrophically in flat bright regions
//   (62500 - 62500 in fp32 against C2 * 255^2 = 58.5); with it both terms are small where the region is flat.  (a-c) and its products are
//   integers below 2^17: exact in fp32.
//   Identical inputs give code 65534 at every pixel: c_a == c_b, every moment of b has the bits of a's, 2 * (mu * mu) == mu * mu + mu * mu
//   and 2 * s_ab == s_aa + s_bb in fp32 as long as the compiler fuses nothing -- contraction is off in the kernel and every fma of the
//   blur is written out -- so numerator and denominator are bit-equal and the IEEE division gives 1.
// MAE kind (gt_mae_kernel): a thread forms four pixels of a row from aligned dwords: s = sum_c |a_c - b_c|, code (257 * s) / 3.
// A map's codes depend on its own pixel pair alone: tiles are anchored at the image's origin, and no value crosses images.
#include "cs_common.h"
#include "gtsum_shared.h"
#include <math.h>

namespace {

constexpr int kTileW = 64, kTileH = 16, kHalo = 5, kTaps = 2 * kHalo + 1;
constexpr int kRegW = kTileW + 2 * kHalo, kRegH = kTileH + 2 * kHalo;  // 74 x 26 pixels
constexpr int kRowDw = (kRegW * 3 + 3 + 3) / 4;                        // dwords that cover a region row at any misalignment: 57
constexpr int kThreads = 256;
constexpr int kRowsPerThread = kTileH / (kThreads / kTileW);           // 4

struct GtTaps {
  float g[kTaps];
};

// the dword at p (4-byte aligned) as far as it lies inside [lo, hi), the image's own bytes; what lies outside reads as 0 and is not touched
__device__ __forceinline__ uint32_t dword_within(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (p + i >= lo && p + i < hi) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the stored SSIM sample of a pixel from the sum of its three channels' terms: one expression for the map form and the sums form
__device__ __forceinline__ int ssim_code(float acc) {
#pragma clang fp contract(off)
  const float v = (acc / 3.0f + 1.0f) * 32767.0f;
  return (int)fminf(fmaxf(v, 0.0f), 65535.0f);
}

// SUMS = false: the map form, codes stored to `out`.  SUMS = true: the same codes, never stored: with the MAE code of the same pixel (formed from
// the bytes the tile holds in LDS) they go into the frame's four sums (cs_op_gt_metric_sums_u8), `out` is not touched.
template <bool SUMS>
__global__ __launch_bounds__(kThreads) void gt_ssim_kernel(const uint8_t* __restrict__ render, const uint8_t* __restrict__ gt, int H, int W,
                                                           long long image_stride, GtTaps taps, uint16_t* __restrict__ out, int out_ld,
                                                           unsigned long long* __restrict__ sums) {
#pragma clang fp contract(off)  // see the head of the file: numerator and denominator must not be fused differently
  __shared__ uint32_t px[2][kRegH][kRowDw];
  __shared__ float plane[5][kRegH][kTileW];
  __shared__ int csum[6];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, b = blockIdx.z;
  const uint8_t* img[2] = {render + (long long)b * image_stride, gt + (long long)b * image_stride};
  const long long img_bytes = (long long)H * W * 3;
  const int xs = x0 - kHalo > 0 ? x0 - kHalo : 0;                          // first and one-past-last image column of the region
  const int xe = x0 + kTileW + kHalo < W ? x0 + kTileW + kHalo : W;
  if (t < 6) csum[t] = 0;

  // a. both images' bytes of the region, once
  for (int i = t; i < 2 * kRegH * kRowDw; i += kThreads) {
    const int k = i % kRowDw, r = (i / kRowDw) % kRegH, im = i / (kRowDw * kRegH);
    const int gy = y0 - kHalo + r;
    if (gy < 0 || gy >= H) continue;
    const uint8_t* g0 = img[im] + ((long long)gy * W + xs) * 3;
    const uint8_t* g1 = img[im] + ((long long)gy * W + xe) * 3;
    const uint8_t* p = g0 - ((uintptr_t)g0 & 3) + 4 * k;
    if (p >= g1) continue;
    px[im][r][k] = dword_within(p, img[im], img[im] + img_bytes);
  }
  __syncthreads();
  const uint8_t* bytes[2] = {reinterpret_cast<const uint8_t*>(&px[0][0][0]), reinterpret_cast<const uint8_t*>(&px[1][0][0])};
  // byte offset of pixel (region row r, image column xs) in bytes[im]: the row's dwords start at its first byte's aligned address
  auto row_off = [&](int im, int r) -> int {
    const int gy = y0 - kHalo + r;
    const uint8_t* g0 = img[im] + ((long long)gy * W + xs) * 3;
    return r * kRowDw * 4 + (int)((uintptr_t)g0 & 3);
  };

  // b. the shifts: rounded mean of the tile's own pixels, per image and channel
  {
    int s[6] = {0, 0, 0, 0, 0, 0};
    for (int q = t; q < kTileH * kTileW; q += kThreads) {
      const int yy = q / kTileW, xx = q % kTileW;
      if (y0 + yy < H && x0 + xx < W) {
        const int r = yy + kHalo, col = (x0 + xx - xs) * 3;
        const int oa = row_off(0, r) + col, ob = row_off(1, r) + col;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[c] += bytes[0][oa + c];
          s[3 + c] += bytes[1][ob + c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int v = wave_sum(s[c]);
      if ((t & 63) == 0) atomicAdd(&csum[c], v);
    }
  }
  __syncthreads();
  const int cnt = (H - y0 < kTileH ? H - y0 : kTileH) * (W - x0 < kTileW ? W - x0 : kTileW);
  const float C1 = 0.01f * 0.01f * 65025.0f, C2 = 0.03f * 0.03f * 65025.0f;

  const int ox = t % kTileW, oy = (t / kTileW) * kRowsPerThread;
  float acc[kRowsPerThread];
#pragma unroll
  for (int o = 0; o < kRowsPerThread; ++o) acc[o] = 0.f;

  for (int ch = 0; ch < 3; ++ch) {
    const int ca = (csum[ch] + cnt / 2) / cnt, cb = (csum[3 + ch] + cnt / 2) / cnt;
    // c1. width pass
    for (int i = t; i < kRegH * kTileW; i += kThreads) {
      const int r = i / kTileW, x = i % kTileW;
      const int gy = y0 - kHalo + r;
      const bool row_ok = gy >= 0 && gy < H;
      const int oa = row_ok ? row_off(0, r) + ch : 0, ob = row_ok ? row_off(1, r) + ch : 0;
      float sa = 0.f, sb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const int gx = x0 - kHalo + x + k;
        const bool ok = row_ok && gx >= 0 && gx < W;
        const int col = ok ? (gx - xs) * 3 : 0;
        const int va = ok ? (int)bytes[0][oa + col] : 0, vb = ok ? (int)bytes[1][ob + col] : 0;
        const float da = (float)(va - ca), db = (float)(vb - cb), w = taps.g[k];
        sa = __builtin_fmaf(w, da, sa);
        sb = __builtin_fmaf(w, db, sb);
        saa = __builtin_fmaf(w, da * da, saa);
        sbb = __builtin_fmaf(w, db * db, sbb);
        sab = __builtin_fmaf(w, da * db, sab);
      }
      plane[0][r][x] = sa;
      plane[1][r][x] = sb;
      plane[2][r][x] = saa;
      plane[3][r][x] = sbb;
      plane[4][r][x] = sab;
    }
    __syncthreads();
    // c2. height pass: this thread's column, rows oy .. oy + 3
    float m[5][kRowsPerThread];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      float v[kRowsPerThread + kTaps - 1];
#pragma unroll
      for (int j = 0; j < kRowsPerThread + kTaps - 1; ++j) v[j] = plane[p][oy + j][ox];
#pragma unroll
      for (int o = 0; o < kRowsPerThread; ++o) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) s = __builtin_fmaf(taps.g[k], v[o + k], s);
        m[p][o] = s;
      }
    }
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
      const float ma = m[0][o], mb = m[1][o];
      const float mua = ma + (float)ca, mub = mb + (float)cb;
      const float saa = m[2][o] - ma * ma, sbb = m[3][o] - mb * mb, sab = m[4][o] - ma * mb;
      const float num = (2.0f * (mua * mub) + C1) * (2.0f * sab + C2);
      const float den = (mua * mua + mub * mub + C1) * (saa + sbb + C2);
      acc[o] = acc[o] + num / den;
    }
    __syncthreads();  // the next channel's width pass overwrites the planes
  }

  // d. codes
  const int gx = x0 + ox;
  if constexpr (!SUMS) {
    if (gx < W) {
#pragma unroll
      for (int o = 0; o < kRowsPerThread; ++o) {
        const int gy = y0 + oy + o;
        if (gy >= H) break;
        out[((long long)b * H + gy) * out_ld + gx] = (uint16_t)ssim_code(acc[o]);
      }
    }
  } else {
    // a thread without a pixel inside the image adds zeros and still arrives at the barrier of cs_sums_block_add
    __shared__ unsigned long long red[kThreads / 64][4];
    uint32_t s1 = 0, s2 = 0, s3 = 0;  // at most four codes each
    unsigned long long s4 = 0;
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
      const int gy = y0 + oy + o;
      if (gx < W && gy < H) {
        const uint32_t cs = (uint32_t)ssim_code(acc[o]);
        const int r = oy + o + kHalo, col = (gx - xs) * 3;
        const int oa = row_off(0, r) + col, ob = row_off(1, r) + col;
        int s = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int va = bytes[0][oa + c], vb = bytes[1][ob + c];
          s += va > vb ? va - vb : vb - va;
        }
        const uint32_t cm = (uint32_t)((257 * s) / 3);  // gt_mae_kernel's code
        s1 += cs;
        s2 += cs < 32767u ? 32767u : (cs > 65534u ? 65534u : cs);
        s3 += cm;
        s4 += (unsigned long long)(cm * cm);
      }
    }
    const unsigned long long v[4] = {s1, s2, s3, s4};
    cs_sums_block_add<kThreads / 64>(v, red, sums + 4 * (long long)b);
  }
}

constexpr int kMaePx = 4;  // pixels per thread: 12 bytes of each image

__global__ __launch_bounds__(kThreads) void gt_mae_kernel(const uint8_t* __restrict__ render, const uint8_t* __restrict__ gt, int H, int W,
                                                          long long image_stride, uint16_t* __restrict__ out, int out_ld) {
  const int x = (blockIdx.x * kThreads + threadIdx.x) * kMaePx, y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const int n = W - x < kMaePx ? W - x : kMaePx;
  const long long img_bytes = (long long)H * W * 3;
  uint32_t e[2][3];
#pragma unroll
  for (int im = 0; im < 2; ++im) {
    const uint8_t* base = (im == 0 ? render : gt) + (long long)b * image_stride;
    const uint8_t* g0 = base + ((long long)y * W + x) * 3;
    const int mis = (int)((uintptr_t)g0 & 3);
    const uint8_t* p = g0 - mis;
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = (j < 3 || mis) ? dword_within(p + 4 * j, base, base + img_bytes) : 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) e[im][j] = (uint32_t)((((uint64_t)d[j + 1] << 32) | d[j]) >> (8 * mis));
  }
  uint16_t code[kMaePx];
#pragma unroll
  for (int i = 0; i < kMaePx; ++i) {
    int s = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int k = 3 * i + c;
      const int va = (e[0][k / 4] >> (8 * (k % 4))) & 255, vb = (e[1][k / 4] >> (8 * (k % 4))) & 255;
      s += va > vb ? va - vb : vb - va;
    }
    code[i] = (uint16_t)((257 * s) / 3);
  }
  uint16_t* o = out + ((long long)b * H + y) * out_ld + x;
  if (n == kMaePx && ((uintptr_t)o & 7) == 0) {
    *reinterpret_cast<uint2*>(o) = make_uint2(code[0] | ((uint32_t)code[1] << 16), code[2] | ((uint32_t)code[3] << 16));
  } else {
#pragma unroll
    for (int i = 0; i < kMaePx; ++i)
      if (i < n) o[i] = code[i];
  }
}

// 11 x 11 Gaussian, sigma 1.5, as the outer product of the 11 taps normalised to sum 1 (fp64, then rounded)
GtTaps gt_taps() {
  GtTaps taps;
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double d = k - kHalo;
    g[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < kTaps; ++k) taps.g[k] = (float)(g[k] / sum);
  return taps;
}

}  // namespace

// the largest H and W the two grids take (rows and 16-row tiles ride in gridDim.y)
extern "C" int cs_gtmap_max_side() { return 65535; }

// kind 0 = SSIM, 1 = MAE (CS_GTMAP_*); arguments are checked by the caller (ops.hip)
extern "C" hipError_t cs_gtmap_launch(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride, int kind, uint16_t* out,
                                      int out_ld, hipStream_t st) {
  if (kind == 1) {
    hipLaunchKernelGGL(gt_mae_kernel, dim3((W + kThreads * kMaePx - 1) / (kThreads * kMaePx), H, B), dim3(kThreads), 0, st, render, gt, H, W,
                       image_stride, out, out_ld);
    return hipGetLastError();
  }
  const GtTaps taps = gt_taps();
  hipLaunchKernelGGL(gt_ssim_kernel<false>, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, B), dim3(kThreads), 0, st, render, gt, H,
                     W, image_stride, taps, out, out_ld, (unsigned long long*)nullptr);
  return hipGetLastError();
}

// the four sums of cs_op_gt_metric_sums_u8 per pair, zeroed on the stream ahead of the one launch; arguments are checked by the caller (ops.hip)
extern "C" hipError_t cs_gtsums_launch(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride, uint64_t* sums,
                                       hipStream_t st) {
  hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * 4 * sizeof(uint64_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gt_ssim_kernel<true>, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, B), dim3(kThreads), 0, st, render, gt, H,
                     W, image_stride, gt_taps(), (uint16_t*)nullptr, 0, reinterpret_cast<unsigned long long*>(sums));
  return hipGetLastError();
}
