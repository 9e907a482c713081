// What the two JPEG entropy kernels share (jpegdec.hip: baseline, jpegprog.hip: progressive): the call's arguments, the plane geometry, the
// wave-uniform bit reader with its FF00 / marker handling, the canonical Huffman tables (build, refusals, 9-bit primary lookup, decode) and the
// ballot pass that finds a scan's restart markers and its end.  Everything here is inlined into the kernel that uses it.
#pragma once

#include "cs_common.h"

#define CS_JPGDEC_THREADS 256
#define CS_JPGDEC_PB 9  // bits of the primary lookup
#define CS_JPGDEC_PROGRESSIVE 1  // CS_JPEG_PROGRESSIVE
#define CS_JPGDEC_MAX_SCANS 32
#define CS_JPGDEC_PENDING 0xFFFFFFFFu  // status word of a progressive file between the two entropy launches of one call

struct CsJpgDecArgs {
  const uint8_t* files;
  const unsigned long long* file_offsets;
  const uint32_t* file_lengths;
  unsigned long long files_bytes;
  int H, W;
  uint8_t* pixels;
  long long image_stride;
  uint32_t* status;
  uint32_t* info;  // workspace: 4 words per file, what the entropy stage read from it (components, luma sampling)
  uint32_t* rst;   // workspace: rst_slot restart-marker positions per file
  unsigned long long rst_slot;
  int16_t* coef;  // workspace: blocks_slot * 64 coefficients per file
  uint8_t* samples;  // workspace: blocks_slot * 64 samples per file
  unsigned long long blocks_slot;
  int flags;           // CS_JPGDEC_PROGRESSIVE: the baseline kernel leaves a SOF2 file to jpegprog.hip
  int levels;          // progressive: 1 the level schedule, 0 one scan per level
  uint32_t* scan_rst;  // progressive workspace: CS_JPGDEC_MAX_SCANS * rst_slot restart-marker positions per file
};

// jpegprog.hip: the progressive entropy launch, between the baseline entropy launch and the IDCT of one call
hipError_t cs_jpgprog_launch(const CsJpgDecArgs& a, int I, hipStream_t st);

namespace {

// status words (include/crossscore_hip.h: CS_JPGDEC_*)
enum { ST_OK = 0, ST_FRAMING = 1, ST_HEADER = 2, ST_TABLE = 3, ST_CODE = 4, ST_SYMBOL = 5, ST_EXHAUSTED = 6, ST_RESTART = 7, ST_SCAN = 8 };

// planes of one file: component c has bw[c] x bh[c] blocks, its first at block off[c]
struct Geometry {
  int ncomp, hs, vs, mcux, mcuy;
  int bw[3], bh[3];
  uint32_t off[3], nblocks;
};

__device__ __forceinline__ Geometry geometry(int H, int W, int ncomp, int hs, int vs) {
  Geometry g;
  g.ncomp = ncomp; g.hs = hs; g.vs = vs;
  g.mcux = (W + 8 * hs - 1) / (8 * hs);
  g.mcuy = (H + 8 * vs - 1) / (8 * vs);
  g.bw[0] = g.mcux * hs; g.bh[0] = g.mcuy * vs;
  g.bw[1] = g.bw[2] = g.mcux; g.bh[1] = g.bh[2] = g.mcuy;
  g.off[0] = 0;
  g.off[1] = (uint32_t)(g.bw[0] * g.bh[0]);
  g.off[2] = g.off[1] + (uint32_t)(g.mcux * g.mcuy);
  g.nblocks = ncomp == 1 ? g.off[1] : g.off[2] + (uint32_t)(g.mcux * g.mcuy);
  return g;
}

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// orders one wave's LDS traffic: what its lanes wrote before is what they read behind
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

__device__ const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ void zigzag_to_lds(uint8_t* zz_lds, int tid) {
  if (tid < 64) zz_lds[tid] = kZigzag[tid];
}

// ---- canonical Huffman tables, in LDS arrays the kernel owns
struct Huff {
  uint16_t* look;   // [1 << CS_JPGDEC_PB]: symbol | length << 8, 0 = walk the canonical code
  uint32_t* first;  // [17] per code length: first code
  uint16_t* cnt;    // [17] ... number of codes
  uint16_t* start;  // [17] ... index of its first symbol
  uint8_t* syms;    // [256]
};

// One table definition of a DHT segment, by one thread: the counts at file[p + 1 .. p + 16], the symbols behind them, all below `send`.
// 0 and the number of symbols, or ST_TABLE.  Reads below send only.
__device__ __forceinline__ int huff_define(const Huff& h, const uint8_t* file, uint32_t p, uint32_t send, uint32_t* nsym) {
  uint32_t total = 0, code = 0;
  for (int l = 1; l <= 16; ++l) {
    const uint32_t c = file[p + l];
    h.cnt[l] = (uint16_t)c;
    h.first[l] = code;
    h.start[l] = (uint16_t)total;
    total += c;
    code += c;
    if (code > (1u << l)) return ST_TABLE;  // more codes than the length allows
    code <<= 1;
  }
  if (total > 256u || 17u + total > send - p) return ST_TABLE;
  for (uint32_t j = 0; j < total; ++j) h.syms[j] = file[p + 17 + j];
  *nsym = total;
  return ST_OK;
}

// the primary lookup of a table of n symbols, by `threads` threads of which this is number t; look[] was zeroed before
__device__ __forceinline__ void huff_fill_lookup(const Huff& h, int n, int t, int threads) {
  for (int j = t; j < n; j += threads) {
    int l = 1;
    while (l < 16 && j >= (int)h.start[l] + (int)h.cnt[l]) ++l;
    if (l <= CS_JPGDEC_PB) {
      const uint32_t code = h.first[l] + (uint32_t)(j - (int)h.start[l]);
      const uint32_t lo = code << (CS_JPGDEC_PB - l), span = 1u << (CS_JPGDEC_PB - l);
      for (uint32_t k = 0; k < span && lo + k < (1u << CS_JPGDEC_PB); ++k) h.look[lo + k] = (uint16_t)(h.syms[j] | ((uint32_t)l << 8));
    }
  }
}

// ---- the bit reader of one wave: wave-uniform state.  bb holds nb valid bits, the next one at bit nb - 1; the last `fake` of them are zeros
// handed out behind the end of the interval (a marker, or `end`).
struct Bits {
  unsigned long long bb;
  int nb, fake;
  uint32_t pos, end, flen, wbase;
  bool eof;
  const uint8_t* file;
  uint32_t* win;
};

__device__ __forceinline__ void load_window(Bits& r, int lane) {
  wave_sync();
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t idx = r.wbase + 4u * (uint32_t)lane + (uint32_t)j;
    if (idx < r.flen) w |= (uint32_t)r.file[idx] << (8 * j);
  }
  r.win[lane] = w;
  wave_sync();
}

__device__ __forceinline__ uint32_t window_word(Bits& r, uint32_t p, int lane) {  // the aligned word that holds byte p
  if (p - r.wbase >= 256u) {
    r.wbase = p & ~3u;
    load_window(r, lane);
  }
  return rfl(r.win[(p - r.wbase) >> 2]);
}

__device__ __forceinline__ uint32_t get_byte(Bits& r, uint32_t p, int lane) { return (window_word(r, p, lane) >> (8u * (p & 3u))) & 255u; }

__device__ __forceinline__ void start_interval(Bits& r, uint32_t start, uint32_t end, int lane) {
  r.bb = 0; r.nb = 0; r.fake = 0; r.pos = start; r.end = end; r.eof = false;
  r.wbase = start & ~3u;
  load_window(r, lane);
}

// at least 57 valid bits afterwards
__device__ __forceinline__ void refill(Bits& r, int lane) {
  if (r.nb <= 32 && !r.eof && (r.pos & 3u) == 0u && r.end - r.pos >= 4u && r.pos < r.end) {
    const uint32_t w = window_word(r, r.pos, lane);
    const uint32_t t = ~w;
    if (((t - 0x01010101u) & ~t & 0x80808080u) == 0u) {  // no FF among the four bytes
      r.bb = (r.bb << 32) | (unsigned long long)__builtin_bswap32(w);
      r.nb += 32;
      r.pos += 4u;
    }
  }
  while (r.nb <= 56) {
    if (r.eof || r.pos >= r.end) {
      r.eof = true;
      r.bb <<= 8;
      r.nb += 8;
      r.fake += 8;
      continue;
    }
    const uint32_t b = get_byte(r, r.pos, lane);
    if (b == 0xFFu) {
      const uint32_t b2 = r.pos + 1u < r.end ? get_byte(r, r.pos + 1u, lane) : 0xFFu;
      if (b2 != 0u) { r.eof = true; continue; }  // a marker: the interval's data ends here
      r.pos += 2u;
    } else {
      r.pos += 1u;
    }
    r.bb = (r.bb << 8) | (unsigned long long)b;
    r.nb += 8;
  }
}

__device__ __forceinline__ uint32_t take(Bits& r, int n) {  // n <= 16 bits that refill() has made available
  r.nb -= n;
  return (uint32_t)(r.bb >> r.nb) & ((1u << n) - 1u);
}

// one symbol of a table: the primary lookup, else the canonical walk.  -1: the next 16 bits are no code of the table.
__device__ __forceinline__ int decode_sym(const Huff& h, Bits& r) {
  const uint32_t w16 = (uint32_t)(r.bb >> (r.nb - 16)) & 0xffffu;
  const uint32_t e = rfl(h.look[w16 >> (16 - CS_JPGDEC_PB)]);
  if (e) {
    r.nb -= (int)(e >> 8);
    return (int)(e & 255u);
  }
  for (int l = CS_JPGDEC_PB + 1; l <= 16; ++l) {
    const uint32_t code = w16 >> (16 - l);
    const uint32_t f = rfl(h.first[l]), c = rfl(h.cnt[l]);
    if (code >= f && code - f < c) {
      r.nb -= l;
      return (int)rfl(h.syms[rfl(h.start[l]) + (code - f)]);
    }
  }
  return -1;
}

__device__ __forceinline__ int extend(uint32_t v, int n) { return v < (1u << (n - 1)) ? (int)v - (1 << n) + 1 : (int)v; }
__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// ---- the restart markers of one scan, in file order, by the whole workgroup (it holds __syncthreads; every thread comes through with the same
// arguments).  The bytes from `scan` on are searched up to the first marker that is neither FF00, a fill FF nor RSTn: scan_end is its position
// (flen when there is none).  The positions of the first nint - 1 RSTn before it go to rst[]; `count` is how many there were, `misnumbered`
// is set in a thread that saw one out of sequence.  wcnt / wterm: 2 x 4 words of LDS.
__device__ __forceinline__ void restart_positions(const uint8_t* file, uint32_t flen, uint32_t scan, uint32_t nint, uint32_t* rst, uint32_t (*wcnt)[4],
                                                  uint32_t (*wterm)[4], int tid, int lane, int wave, uint32_t& scan_end, uint32_t& count,
                                                  int& misnumbered) {
  int par = 0;
  for (uint32_t base = scan; base < flen; base += CS_JPGDEC_THREADS, par ^= 1) {
    const uint32_t i = base + (uint32_t)tid;
    const uint32_t b0 = i < flen ? file[i] : 0u, b1 = i + 1u < flen && i + 1u > i ? file[i + 1u] : 0u;
    const bool is_rst = b0 == 0xFFu && (b1 & 0xF8u) == 0xD0u;
    const bool is_term = b0 == 0xFFu && b1 != 0u && b1 != 0xFFu && !is_rst;
    unsigned long long mr = __ballot(is_rst);
    const unsigned long long mt = __ballot(is_term);
    uint32_t term = 0xffffffffu;
    if (mt) {
      const int f = __ffsll((long long)mt) - 1;
      mr &= (1ull << f) - 1ull;
      term = base + 64u * (uint32_t)wave + (uint32_t)f;
    }
    if (lane == 0) { wcnt[par][wave] = (uint32_t)__popcll(mr); wterm[par][wave] = term; }
    __syncthreads();
    uint32_t tpos = 0xffffffffu, before = count, all = count;
    for (int w = 0; w < 4; ++w) {
      tpos = min(tpos, wterm[par][w]);
      const uint32_t c = (base + 64u * (uint32_t)w > tpos) ? 0u : wcnt[par][w];
      if (w < wave) before += c;
      all += c;
    }
    if (is_rst && i < tpos) {
      const uint32_t idx = before + (uint32_t)__popcll(mr & ((1ull << lane) - 1ull));
      if (idx < nint - 1u) {
        rst[idx] = i;
        if (((b1 - 0xD0u) & 7u) != (idx & 7u)) misnumbered = 1;
      }
    }
    count = all;
    if (tpos != 0xffffffffu) { scan_end = tpos; break; }  // uniform: every thread sees the same tpos
  }
}

}  // namespace
