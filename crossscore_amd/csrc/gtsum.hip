// Per-frame integer sums of stored ground-truth metric maps (gfx950): B pairs of uint16 maps (SSIM codes, MAE codes) in, per frame the four
// unsigned 64-bit sums out that the ground-truth score summary is a rational function of:
//   S1 = sum c_ssim   S2 = sum clamp(c_ssim, 32767, 65534)   S3 = sum c_mae   S4 = sum c_mae^2
// Streaming, 4 bytes per pixel.  A workgroup of four waves owns 16 rows of one frame, a wave one row at a time (waves take neighbouring rows).
// Of a row only [row, row + W) is read: single samples up to the first 16-byte boundary, 16-byte loads of eight samples from there, single
// samples for what is left (both ends are below eight samples, one lane each); the two maps are aligned independently.
// Per thread S1..S3 are 32-bit: a thread sees at most 4 rows x (ceil(8192 / 64) x 8 + 2) = 4104 samples of one map (W <= 65535), and
// 4104 x 65535 < 2^32.  c^2 <= 65535^2 < 2^32 is formed in 32 bits and added in 64.  Then cs_sums_block_add (gtsum_shared.h).
// No thread leaves before the barrier in there: rows past H are skipped by the loop, not by a return.
#include "cs_common.h"
#include "gtsum_shared.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kRowsPerBlock = 16;

template <bool SSIM>
__device__ __forceinline__ void add_code(uint32_t c, uint32_t& plain, uint32_t& clipped, unsigned long long& squares) {
  plain += c;
  if (SSIM)
    clipped += c < 32767u ? 32767u : (c > 65534u ? 65534u : c);  // the clip to [0, 1] of c / 32767 - 1 (code 65535 reads as 1.00003)
  else
    squares += (unsigned long long)(c * c);
}

template <bool SSIM>
__device__ __forceinline__ void row_sums(const uint16_t* __restrict__ row, int W, int lane, uint32_t& plain, uint32_t& clipped,
                                         unsigned long long& squares) {
  int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);  // samples before the first 16-byte boundary: 0..7
  if (head > W) head = W;
  const int nvec = (W - head) >> 3;
  const int tail0 = head + (nvec << 3);
  if (lane < head) add_code<SSIM>(row[lane], plain, clipped, squares);
  if (lane < W - tail0) add_code<SSIM>(row[tail0 + lane], plain, clipped, squares);
  const uint4* v = reinterpret_cast<const uint4*>(row + head);
  for (int i = lane; i < nvec; i += 64) {
    const uint4 d = v[i];
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      add_code<SSIM>(w[j] & 0xFFFFu, plain, clipped, squares);
      add_code<SSIM>(w[j] >> 16, plain, clipped, squares);
    }
  }
}

__global__ __launch_bounds__(kThreads) void map_sums_kernel(const uint16_t* __restrict__ ssim, const uint16_t* __restrict__ mae, int H, int W,
                                                            int row_elems, long long image_stride, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long red[kWaves][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int y0 = blockIdx.x * kRowsPerBlock;
  uint32_t s1 = 0, s2 = 0, s3 = 0, none32 = 0;
  unsigned long long s4 = 0, none64 = 0;
  for (int r = wave; r < kRowsPerBlock && y0 + r < H; r += kWaves) {
    const long long at = (long long)b * image_stride + (long long)(y0 + r) * row_elems;
    row_sums<true>(ssim + at, W, lane, s1, s2, none64);
    row_sums<false>(mae + at, W, lane, s3, none32, s4);
  }
  const unsigned long long v[4] = {s1, s2, s3, s4};
  cs_sums_block_add<kWaves>(v, red, sums + 4 * (long long)b);
}

}  // namespace

// arguments are checked by the caller (ops.hip); sums is zeroed on the stream ahead of the kernel
extern "C" hipError_t cs_metric_map_sums_launch(const uint16_t* ssim, const uint16_t* mae, int B, int H, int W, int row_elems,
                                                long long image_stride, uint64_t* sums, hipStream_t st) {
  hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * 4 * sizeof(uint64_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_sums_kernel, dim3((H + kRowsPerBlock - 1) / kRowsPerBlock, B), dim3(kThreads), 0, st, ssim, mae, H, W, row_elems,
                     image_stride, reinterpret_cast<unsigned long long*>(sums));
  return hipGetLastError();
}
