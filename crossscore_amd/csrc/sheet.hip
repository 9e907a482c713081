// Preview sheet compositor (gfx950): paints up to 48 panels -- fills, area-resampled images, the blend of two
// images, a colour ramp, frames and 5 x 7 text -- into one (canvas_h, canvas_w, 3) uint8 canvas in ONE launch (include/crossscore_hip.h states
// the definition).  Integers throughout.
//
// The panels travel as kernel arguments.  The grid runs over 64 x 64 canvas tiles.  A workgroup keeps its tile in LDS, starts it at zero, paints
// the panels that meet the tile into it in call order (a barrier between two panels, so a later one covers an earlier one whatever the thread
// that painted it), and then stores every canvas byte of the tile exactly once: no atomics and no read of the canvas, so nothing outside the
// canvas is touched and the result cannot depend on the order of workgroups.  An LDS row is shifted by the low two bits of its canvas address,
// so whole aligned dwords go out and only the ragged ends of a row are byte stores.
//
// IMAGE / BLEND (exact area resampling, out = (S + area / 2) / area with S = sum wy wx v): separable.  The source rows the tile's destination
// rows reach are taken in chunks of 16.  Horizontal: a wave owns a source row at a time, stages its bytes into LDS 256 pixels at a time
// with lane k loading byte k, k + 64, ... (BLEND forms (a + b + 1) >> 1 here, per source pixel), then lane c sums the pixels of destination
// column c with their weights wx; every source row is summed once.  Vertical: thread (column, row group) adds wy x the chunk's horizontal sums
// into its destination rows' accumulators (LDS, u32: S <= 255 x 4096 x 4096 < 2^32).  The last step divides.
#include "../../include/crossscore_hip.h"  // plain C: the CS_SHEET_* kinds
#include "cs_common.h"
#include "sheet_font.h"

namespace {

constexpr int kTile = 64, kThreads = 256, kWaves = kThreads / 64;
constexpr int kPitch = kTile * 3 + 8;  // bytes of an LDS tile row: 192, up to 3 of shift, rounded to dwords
constexpr int kPiece = 256;            // source pixels a wave stages at a time
constexpr int kRows = 16;              // source rows of a chunk: their horizontal sums are in LDS together

__device__ const uint8_t kFont[CS_SHEET_GLYPHS][7] = {CS_SHEET_FONT_ROWS};

struct Tile {
  uint8_t* bytes;  // kTile rows of kPitch
  int base3, cw3;  // the low two bits of the canvas address of the tile's first byte, and of a canvas row's length
  __device__ __forceinline__ int shift(int r) const { return (base3 + r * cw3) & 3; }
  __device__ __forceinline__ void put(int r, int c, uint32_t r8, uint32_t g8, uint32_t b8) const {
    uint8_t* d = bytes + r * kPitch + shift(r) + c * 3;
    d[0] = (uint8_t)r8; d[1] = (uint8_t)g8; d[2] = (uint8_t)b8;
  }
};

// overlap of [i * d, (i + 1) * d) with [j * s, (j + 1) * s): the weight of source index i in destination index j (s source, d destination size)
__device__ __forceinline__ uint32_t overlap(int i, int j, int s, int d) {
  const int lo = max(i * d, j * s), hi = min((i + 1) * d, (j + 1) * s);
  return (uint32_t)max(0, hi - lo);
}

// The part [ry0, ry1) x [cx0, cx1) (panel coordinates, at most 64 x 64) of an IMAGE / BLEND panel into the tile at (y0, x0).  Every loop bound a
// barrier sits in is the same in all threads of the workgroup.
__device__ void resample(const CsSheetPanel& q, const Tile& t, int y0, int x0, int ry0, int ry1, int cx0, int cx1, uint8_t (*stage)[kPiece * 3],
                         uint32_t (*hs)[kTile * 3], uint32_t (*acc)[kTile * 3]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sh = q.sh, sw = q.sw, dh = q.h, dw = q.w;
  const int nr = ry1 - ry0, nc = cx1 - cx0;
  const bool blend = q.kind == CS_SHEET_BLEND;
  for (int i = tid; i < nr * kTile * 3; i += kThreads) acc[0][i] = 0;
  const int sx0 = (cx0 * sw) / dw, sx1 = (cx1 * sw + dw - 1) / dw;  // the source columns and rows this part reaches
  const int sy0 = (ry0 * sh) / dh, sy1 = (ry1 * sh + dh - 1) / dh;
  const int j = cx0 + lane;                                        // this lane's destination column and its source columns [a, b)
  const int a = (j * sw) / dw, b = ((j + 1) * sw + dw - 1) / dw;
  for (int ci0 = sy0; ci0 < sy1; ci0 += kRows) {
    const int ci1 = min(ci0 + kRows, sy1);
    for (int k = 0; ci0 + k * kWaves < ci1; ++k) {
      const int i = ci0 + k * kWaves + wave;
      const bool live = i < ci1;
      uint32_t h0 = 0, h1 = 0, h2 = 0;
      for (int p0 = sx0; p0 < sx1; p0 += kPiece) {
        const int p1 = min(p0 + kPiece, sx1), nb = (p1 - p0) * 3;
        if (live) {
          const uint8_t* s = q.src + (size_t)i * q.row_bytes + (size_t)p0 * 3;
          if (blend) {
            const uint8_t* s2 = q.src2 + (size_t)i * q.row_bytes2 + (size_t)p0 * 3;
            for (int v = lane; v < nb; v += 64) stage[wave][v] = (uint8_t)(((uint32_t)s[v] + s2[v] + 1u) >> 1);
          } else {
            for (int v = lane; v < nb; v += 64) stage[wave][v] = s[v];
          }
        }
        __syncthreads();
        if (live && lane < nc) {
          for (int ix = max(a, p0); ix < min(b, p1); ++ix) {
            const uint32_t wx = overlap(ix, j, sw, dw);
            const uint8_t* px = stage[wave] + (ix - p0) * 3;
            h0 += wx * px[0]; h1 += wx * px[1]; h2 += wx * px[2];
          }
        }
        __syncthreads();
      }
      if (live && lane < nc) {
        uint32_t* h = hs[i - ci0] + lane * 3;
        h[0] = h0; h[1] = h1; h[2] = h2;
      }
    }
    __syncthreads();
    const int jlo = max(ry0, (ci0 * dh) / sh), jhi = min(ry1, (ci1 * dh + sh - 1) / sh);  // the destination rows this chunk reaches
    if (lane < nc) {
      for (int jr = jlo + wave; jr < jhi; jr += kWaves) {
        const int i0 = max(ci0, (jr * sh) / dh), i1 = min(ci1, ((jr + 1) * sh + dh - 1) / dh);
        uint32_t v0 = 0, v1 = 0, v2 = 0;
        for (int i = i0; i < i1; ++i) {
          const uint32_t wy = overlap(i, jr, sh, dh);
          const uint32_t* h = hs[i - ci0] + lane * 3;
          v0 += wy * h[0]; v1 += wy * h[1]; v2 += wy * h[2];
        }
        uint32_t* s = acc[jr - ry0] + lane * 3;
        s[0] += v0; s[1] += v1; s[2] += v2;
      }
    }
    __syncthreads();
  }
  const uint32_t area = (uint32_t)sh * (uint32_t)sw, half = area / 2;
  if (lane < nc) {
    for (int r = wave; r < nr; r += kWaves) {
      const uint32_t* s = acc[r] + lane * 3;
      t.put(y0 + r, x0 + lane, (s[0] + half) / area, (s[1] + half) / area, (s[2] + half) / area);
    }
  }
}

__global__ __launch_bounds__(kThreads) void sheet_compose_kernel(const CsSheetPanels panels, int n, uint8_t* __restrict__ canvas, int ch, int cw) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile * kPitch];
  __shared__ uint8_t stage[kWaves][kPiece * 3];
  __shared__ uint32_t hs[kRows][kTile * 3];
  __shared__ uint32_t acc[kTile][kTile * 3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int th = min(kTile, ch - ty0), tw = min(kTile, cw - tx0);
  Tile t;
  t.bytes = tile;
  t.base3 = (int)(((uintptr_t)canvas + ((size_t)ty0 * cw + tx0) * 3) & 3);
  t.cw3 = (cw * 3) & 3;
  for (int i = tid; i < kTile * kPitch / 4; i += kThreads) reinterpret_cast<uint32_t*>(tile)[i] = 0;
  __syncthreads();
  for (int p = 0; p < n; ++p) {
    const CsSheetPanel& q = panels.p[p];
    // the part of the panel inside this tile, in tile coordinates (the same in every thread: a panel that misses the tile is skipped by all)
    const int y0 = max(q.y, ty0) - ty0, y1 = min(q.y + q.h, ty0 + th) - ty0;
    const int x0 = max(q.x, tx0) - tx0, x1 = min(q.x + q.w, tx0 + tw) - tx0;
    if (y0 >= y1 || x0 >= x1) continue;
    const int py = ty0 - q.y, px = tx0 - q.x;  // tile -> panel coordinates
    const uint32_t r8 = q.rgb & 255u, g8 = (q.rgb >> 8) & 255u, b8 = (q.rgb >> 16) & 255u;
    if (q.kind == CS_SHEET_IMAGE || q.kind == CS_SHEET_BLEND) {
      resample(q, t, y0, x0, y0 + py, y1 + py, x0 + px, x1 + px, stage, hs, acc);
    } else {
      const int c = x0 + lane, pc = c + px;
      if (c < x1) {
        for (int r = y0 + wave; r < y1; r += kWaves) {
          const int pr = r + py;
          if (q.kind == CS_SHEET_FILL) {
            t.put(r, c, r8, g8, b8);
          } else if (q.kind == CS_SHEET_RAMP) {
            const uint8_t* e = q.src + (255 - (pr * 256) / q.h) * 3;
            t.put(r, c, e[0], e[1], e[2]);
          } else if (q.kind == CS_SHEET_FRAME) {
            if (pr < q.param || pr >= q.h - q.param || pc < q.param || pc >= q.w - q.param) t.put(r, c, r8, g8, b8);
          } else {  // CS_SHEET_TEXT: cells of 6 x param columns, of which the first 5 x param hold the glyph
            const int cell = pc / (6 * q.param), gx = (pc - cell * 6 * q.param) / q.param, gy = pr / q.param;
            const int glyph = (int)((q.glyphs >> (4 * cell)) & 15u);
            if (gx < 5 && ((kFont[glyph][gy] >> (4 - gx)) & 1)) t.put(r, c, r8, g8, b8);
          }
        }
      }
    }
    __syncthreads();
  }
  // the tile's rows out: byte v of row r is tile[r][shift + v], and canvas byte v of the row sits at an address whose low bits are `shift`
  const int nb = tw * 3;
  for (int r = wave; r < th; r += kWaves) {
    const int sft = t.shift(r);
    uint8_t* g = canvas + ((size_t)(ty0 + r) * cw + tx0) * 3 - sft;  // dword aligned; the first sft bytes are not this row's and are not touched
    const uint8_t* l = tile + r * kPitch;
    const int lo = lane * 4, hi = lo + 4;
    if (lo >= sft && hi <= sft + nb) {
      *reinterpret_cast<uint32_t*>(g + lo) = *reinterpret_cast<const uint32_t*>(l + lo);
    } else {
      for (int v = max(lo, sft); v < min(hi, sft + nb); ++v) g[v] = l[v];
    }
  }
}

}  // namespace

extern "C" hipError_t cs_sheet_launch(const CsSheetPanels* panels, int n, uint8_t* canvas, int ch, int cw, hipStream_t st) {
  const dim3 grid((unsigned)((cw + kTile - 1) / kTile), (unsigned)((ch + kTile - 1) / kTile));
  hipLaunchKernelGGL(sheet_compose_kernel, grid, dim3(kThreads), 0, st, *panels, n, canvas, ch, cw);
  return hipGetLastError();
}
