// PNG encoder on the device (gfx950): integer images in, complete PNG files out.  Every byte of a file -- signature, IHDR, the IDAT chunks
// with the zlib stream, Adler-32, every chunk CRC, IEND -- is produced by the two kernels below; the host copies and writes.
//
// Layout of a file
//   signature | IHDR | IDAT(seg 0: 78 01 + deflate) | IDAT(seg 1) | ... | IDAT(Adler-32, 4 bytes) | IEND
// The filtered scanline stream (a filter-type byte + the row bytes per row, 16-bit samples big-endian) is cut into independent segments of
// CS_PNG_SEG bytes (the last one is whatever remains).  A segment is compressed by one workgroup with no history from other segments: one
// fixed-Huffman block (BTYPE=01) with LZ77 matches inside the segment, or one stored block (BTYPE=00) when that is not shorter.  Every
// segment but the last appends an empty stored block, which byte-aligns the stream (Z_SYNC_FLUSH), so that segments concatenate; the last
// one's block carries BFINAL.  One IDAT chunk per segment makes every chunk CRC a per-segment quantity; the Adler-32 of the whole stream is
// combined from per-segment sums and rides in a last 4-byte IDAT chunk.
//
// Filter: Sub (type 1) for both kinds, on every row.  Filtering reads raw pixels only.
//
// Two opt-in flags (cs_op_png_encode_ex) change what a segment's workgroup emits; without them the bytes are the ones described above.
//   CS_PNG_ADAPTIVE_FILTER  every row takes the filter type (None, Sub, Up, Average, Paeth) whose filtered bytes have the smallest
//      sum of min(f, 256 - f), ties to the lowest type.  A wave scores a whole row from the raw pixels (the row above row 0 is zeros), so the
//      two segments that share a straddling row reach the same type without talking to each other.
//   CS_PNG_DYNAMIC  after the parse the workgroup counts, with LDS integer atomics, the symbols of the parse's tokens and the plain bytes of
//      the segment (the literals-only form), builds a length-limited prefix code for each (png_huff.h: rank sort by (count, symbol), one lane
//      per code set for the serial construction over <= 320 symbols), prices stored / fixed + tokens / dynamic + tokens / dynamic + literals
//      exactly from the counts, and emits the smallest (a later form wins only when strictly smaller in bytes).  No form is longer than the
//      stored one, so cs_png_bound holds as it is.
//
// Kernel 1 (png_segment_kernel, one workgroup per (segment, image)):
//   a. filtered bytes -> LDS; the segment's Adler sums S = sum b_i, T = sum (n - i) b_i
//   b. LZ77 candidates: a 4096-entry hash table over 3-byte prefixes, filled 512 positions at a time (atomicMax: the result does not depend
//      on thread order), plus the fixed distances 1, bytes-per-pixel and one row; longest match (<= 258) wins, ties to the earlier candidate
//   c. greedy parse: the positions reached from 0 by i -> i + (len >= 3 ? len : 1), marked by pointer doubling in 15 rounds
//   d. token code lengths -> prefix sum (wave scans) -> bits OR-ed into an LDS image of the chunk with LDS atomics
//   e. chunk CRC-32: lanes take 36-byte slices through a 256-entry table in LDS, each slice's remainder is multiplied by
//      x^(8 * bytes behind it) mod P with the powers x^(8 * 2^j), and the products are XOR-reduced
//   f. the finished chunk (length, "IDAT", payload, CRC) goes to the segment's staging slot, with (chunk bytes, S, T)
// Kernel 2 (png_assemble_kernel, one workgroup per (segment, image)): the chunk's offset is the sum of the chunk lengths before it; the
//   chunk is copied there.  Segment 0's workgroup also writes signature + IHDR, the last segment's the Adler chunk, IEND and the file length.
// Two launches per call whatever I is; nothing waits for the device.  The bytes of an image depend on its pixels, size and kind alone.
#include "cs_common.h"
#include "png_huff.h"
#include "png_probe.h"

#define CS_PNG_SEG 16384
#define CS_PNG_SLOT (CS_PNG_SEG + 64)   // staging bytes per segment: 16-byte record + chunk (<= 12 + 2 + 5 + SEG) + slack for word reads
#define CS_PNG_FIXED 61                 // signature 8 + IHDR 25 + Adler IDAT 16 + IEND 12
#define CS_PNG_THREADS 512

namespace {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kAdlerMod = 65521u;

__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {  // a * b mod P, reflected representation (x^0 = bit 31)
  uint32_t p = 0;
  for (int k = 31; k >= 0; --k) {
    if ((a >> k) & 1u) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) v ^= __shfl_xor(v, o, 64);
  return v;
}

struct PngGeom {
  int kind, H, W;
  int rb;        // raw bytes per row
  int rl;        // 1 + rb
  int bpp;       // bytes per pixel: 2 (gray16) or 3 (rgb8)
  unsigned total;  // H * rl, the filtered stream's length
  int nseg;
};

// raw byte j (file order: 16-bit samples big-endian) of a row
__device__ __forceinline__ uint32_t raw_byte(const uint8_t* row, int kind, int j) {
  if (kind == 0) {
    const uint16_t s = reinterpret_cast<const uint16_t*>(row)[j >> 1];
    return (j & 1) ? (s & 0xffu) : (s >> 8);
  }
  return row[j];
}

__device__ __forceinline__ uint32_t filtered_byte(const uint8_t* img, const PngGeom& g, unsigned p) {
  const unsigned row = p / (unsigned)g.rl;
  const int col = (int)(p - row * (unsigned)g.rl);
  if (col == 0) return 1u;  // filter type Sub
  const int j = col - 1;
  const uint8_t* r = img + (size_t)row * g.rb;
  const uint32_t a = raw_byte(r, g.kind, j);
  const uint32_t b = j >= g.bpp ? raw_byte(r, g.kind, j - g.bpp) : 0u;
  return (a - b) & 0xffu;
}

// the same with the row's own filter type: ftype[row - r0], chosen by step a0 of the kernel
__device__ __forceinline__ uint32_t filtered_byte_adaptive(const uint8_t* img, const PngGeom& g, unsigned p, const uint8_t* ftype, unsigned r0) {
  const unsigned row = p / (unsigned)g.rl;
  const int col = (int)(p - row * (unsigned)g.rl);
  const int type = ftype[row - r0];
  if (col == 0) return (uint32_t)type;
  const int j = col - 1;
  const uint8_t* r = img + (size_t)row * g.rb;
  const bool left = j >= g.bpp, up = row > 0 && type >= 2;
  const uint32_t x = raw_byte(r, g.kind, j);
  const uint32_t a = left ? raw_byte(r, g.kind, j - g.bpp) : 0u;
  const uint32_t b = up ? raw_byte(r - g.rb, g.kind, j) : 0u;
  const uint32_t c = up && left ? raw_byte(r - g.rb, g.kind, j - g.bpp) : 0u;
  return cs_huff::png_filter(type, x, a, b, c);
}

// four bytes at any byte offset of a word array (little-endian)
__device__ __forceinline__ uint32_t ld32(const uint32_t* w, int p) {
  const uint32_t a = w[p >> 2], b = w[(p >> 2) + 1];
  const int sh = (p & 3) * 8;
  return (uint32_t)((((uint64_t)b << 32) | a) >> sh);
}

__device__ __forceinline__ int match_len(const uint32_t* in32, int i, int c, int maxl) {
  int l = 0;
  while (l < maxl) {
    const uint32_t x = ld32(in32, i + l) ^ ld32(in32, c + l);
    if (x) { l += __builtin_ctz(x) >> 3; break; }
    l += 4;
  }
  return l < maxl ? l : maxl;
}

// fixed-Huffman code of one token, ready for the LSB-first bit stream: value in .x, bit count in .y
__device__ __forceinline__ uint2 token_bits(uint32_t lit, int len, int dist) {
  if (len < 3) {
    if (lit < 144u) return make_uint2(__brev(0x30u + lit) >> 24, 8u);
    return make_uint2(__brev(0x190u + (lit - 144u)) >> 23, 9u);
  }
  uint32_t sym, eb = 0, ev = 0;
  if (len <= 10) sym = 254u + len;
  else if (len == 258) sym = 285u;
  else {
    const uint32_t l = len - 3;
    eb = (31u - __builtin_clz(l)) - 2u;
    sym = 261u + 4u * eb + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
  }
  uint32_t v, n;
  if (sym < 280u) { v = __brev(sym - 256u) >> 25; n = 7; }
  else { v = __brev(0xC0u + (sym - 280u)) >> 24; n = 8; }
  v |= ev << n; n += eb;
  uint32_t dc, db = 0, dv = 0;
  if (dist <= 4) dc = dist - 1;
  else {
    const uint32_t d = dist - 1;
    db = (31u - __builtin_clz(d)) - 1u;
    dc = 2u * db + 2u + ((d >> db) & 1u);
    dv = d & ((1u << db) - 1u);
  }
  v |= (__brev(dc) >> 27) << n; n += 5;
  v |= dv << n; n += db;
  return make_uint2(v, n);
}

// LDS image of kernel 1 (dynamic): see the offsets below
constexpr int kInBytes = CS_PNG_SEG + 16;                 // filtered bytes + zero padding for ld32
constexpr int kLdBytes = CS_PNG_SEG * 4;                  // per position: len (9 bits) | dist << 9 | reached << 31
constexpr int kUBytes = 2 * (CS_PNG_SEG + 1) + 62;        // hash table (16 KiB), then jump (u16), then the chunk image: 32832 bytes
constexpr int kOutWords = (CS_PNG_SEG + 64) / 4;          // chunk image capacity in words
constexpr int kLdsBytes = kInBytes + kLdBytes + kUBytes + 1024 + 64 + 256;
static_assert(kUBytes % 4 == 0 && kUBytes >= kOutWords * 4 && kUBytes >= 4096 * 4, "union region");

// LDS behind the image above, CS_PNG_DYNAMIC only.  Code sets: 0 = the parse's tokens, 1 = literals only, 2 = the fixed code (lengths preset,
// so that one emitter serves all three); sort trees: 0 = set 0 literal/length, 1 = set 0 distance, 2 = set 1 literal/length.
struct DynLds {
  uint32_t hist[2][cs_huff::kAlpha];
  uint32_t key[3][cs_huff::kLL];
  uint16_t sym[3][cs_huff::kLL];
  uint16_t code[3][cs_huff::kAlpha];
  uint8_t len[3][cs_huff::kAlpha];
  uint32_t hdr[2][cs_huff::kHdrWords];
  cs_huff::HeaderScratch hs[2];
  uint32_t num[3][16];
  uint32_t used[3];
  uint32_t hdrbits[2];
  uint32_t bits[3];  // payload bits with the end-of-block code: set 0, set 1, set 2 with set 0's counts
};
static_assert(kLdsBytes % 16 == 0 && kLdsBytes + sizeof(DynLds) <= 160 * 1024, "LDS of the dynamic form");

template <int FLAGS>
__global__ __launch_bounds__(CS_PNG_THREADS) void png_segment_kernel(const uint8_t* __restrict__ pixels, long long image_stride, PngGeom g,
                                                                     uint8_t* __restrict__ staging) {
  extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];
  uint32_t* in32 = reinterpret_cast<uint32_t*>(png_lds);
  const uint8_t* in8 = png_lds;
  uint32_t* ld = reinterpret_cast<uint32_t*>(png_lds + kInBytes);
  unsigned char* ureg = png_lds + kInBytes + kLdBytes;
  uint32_t* htab = reinterpret_cast<uint32_t*>(ureg);
  uint16_t* jump = reinterpret_cast<uint16_t*>(ureg);
  uint32_t* out32 = reinterpret_cast<uint32_t*>(ureg);
  uint8_t* out8 = ureg;
  uint32_t* crct = reinterpret_cast<uint32_t*>(ureg + kUBytes);
  uint32_t* cpow = crct + 256;                                  // x^(8 * 2^j), j < 16
  uint32_t* red = cpow + 16;                                    // 64 words of reduction scratch

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = CS_PNG_THREADS / 64;
  const int seg = blockIdx.x, img = blockIdx.y;
  const uint8_t* src = pixels + (size_t)img * image_stride;
  const unsigned seg0 = (unsigned)seg * CS_PNG_SEG;
  const int n = (int)min((unsigned)CS_PNG_SEG, g.total - seg0);
  const bool first = seg == 0, last = seg == g.nseg - 1;

  // ---- tables
  if (tid < 256) {
    uint32_t c = tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    crct[tid] = c;
  } else if (tid < 256 + 16) {
    uint32_t p = 0x40000000u;  // x^1
    for (int k = 0; k < (tid - 256) + 3; ++k) p = crc_mulmod(p, p);
    cpow[tid - 256] = p;
  }
  // ---- a0. adaptive filter: a wave scores each row that has bytes in this segment, over the whole row (the types sit in ld's bytes until b)
  const uint8_t* ftype = reinterpret_cast<const uint8_t*>(ld);
  const unsigned row0 = seg0 / (unsigned)g.rl;
  if constexpr ((FLAGS & 2) != 0) {
    const unsigned row1 = (seg0 + (unsigned)n - 1u) / (unsigned)g.rl;
    for (unsigned row = row0 + wv; row <= row1; row += NW) {
      const uint8_t* cur = src + (size_t)row * g.rb;
      uint32_t sc[5] = {0u, 0u, 0u, 0u, 0u};
      for (int j = lane; j < g.rb; j += 64) {
        const bool left = j >= g.bpp, up = row > 0;
        const uint32_t x = raw_byte(cur, g.kind, j);
        const uint32_t a = left ? raw_byte(cur, g.kind, j - g.bpp) : 0u;
        const uint32_t b = up ? raw_byte(cur - g.rb, g.kind, j) : 0u;
        const uint32_t c = up && left ? raw_byte(cur - g.rb, g.kind, j - g.bpp) : 0u;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
          const uint32_t f = cs_huff::png_filter(t, x, a, b, c);
          sc[t] += min(f, 256u - f);
        }
      }
      int best = 0;
      uint32_t best_score = 0xffffffffu;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        for (int o = 32; o >= 1; o >>= 1) sc[t] += __shfl_xor(sc[t], o, 64);
        if (sc[t] < best_score) { best_score = sc[t]; best = t; }
      }
      if (lane == 0) reinterpret_cast<uint8_t*>(ld)[row - row0] = (uint8_t)best;
    }
    __syncthreads();
  }
  // ---- a. filtered bytes, Adler sums
  uint32_t s_sum = 0;
  unsigned long long t_sum = 0;
  for (int w = tid; w < kInBytes / 4; w += CS_PNG_THREADS) {
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = w * 4 + e;
      if (t < n) {
        const uint32_t b = (FLAGS & 2) ? filtered_byte_adaptive(src, g, seg0 + t, ftype, row0) : filtered_byte(src, g, seg0 + t);
        v |= b << (8 * e);
        s_sum += b;
        t_sum += (unsigned long long)(n - t) * b;
      }
    }
    in32[w] = v;
  }
  for (int i = tid; i < 4096; i += CS_PNG_THREADS) htab[i] = 0;
  for (int o = 32; o >= 1; o >>= 1) {
    s_sum += __shfl_xor(s_sum, o, 64);
    t_sum += __shfl_xor(t_sum, o, 64);
  }
  if (lane == 0) { red[wv] = s_sum; red[16 + 2 * wv] = (uint32_t)t_sum; red[16 + 2 * wv + 1] = (uint32_t)(t_sum >> 32); }
  __syncthreads();
  uint32_t adler_s = 0, adler_t = 0;
  if (tid == 0) {
    unsigned long long S = 0, T = 0;
    for (int k = 0; k < NW; ++k) { S += red[k]; T += ((unsigned long long)red[16 + 2 * k + 1] << 32) | red[16 + 2 * k]; }
    adler_s = (uint32_t)(S % kAdlerMod);
    adler_t = (uint32_t)(T % kAdlerMod);
  }
  // ---- b. candidates from the hash table: the latest position of an earlier 512-block with the same 3-byte prefix
  for (int base = 0; base < n; base += CS_PNG_THREADS) {
    const int i = base + tid;
    uint32_t h = 0;
    const bool live = i + 3 <= n;
    if (live) {
      h = ((ld32(in32, i) & 0xffffffu) * 2654435761u) >> 20;
      ld[i] = htab[h];  // position + 1, 0 = none
    } else if (i < n) {
      ld[i] = 0;
    }
    __syncthreads();
    if (live) atomicMax(&htab[h], (uint32_t)(i + 1));
    __syncthreads();
  }
  // longest match per position
  for (int i = tid; i < n; i += CS_PNG_THREADS) {
    const int maxl = min(258, n - i);
    int best = 0, bdist = 0;
    if (maxl >= 3) {
      const int cand[4] = {i - 1, i - g.bpp, i - g.rl, (int)ld[i] - 1};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cand[k];
        if (c >= 0 && best < maxl) {
          const int l = match_len(in32, i, c, maxl);
          if (l > best) { best = l; bdist = i - c; }
        }
      }
      if (best < 3 || (best == 3 && bdist > 4096)) { best = 0; bdist = 0; }
    }
    ld[i] = (uint32_t)best | ((uint32_t)bdist << 9) | (i == 0 ? 0x80000000u : 0u);
  }
  __syncthreads();
  // ---- c. greedy parse by pointer doubling (the hash table is dead: its bytes become the jump array)
  for (int i = tid; i <= n; i += CS_PNG_THREADS) {
    const int l = i < n ? (int)(ld[i] & 0x1ffu) : 0;
    jump[i] = (uint16_t)(i < n ? i + (l >= 3 ? l : 1) : n);
  }
  __syncthreads();
  constexpr int PER = CS_PNG_SEG / CS_PNG_THREADS + 1;
  for (int r = 0; r < 15; ++r) {
    for (int i = tid; i < n; i += CS_PNG_THREADS)
      if (ld[i] & 0x80000000u) {
        const int j = jump[i];
        if (j < n) atomicOr(&ld[j], 0x80000000u);
      }
    __syncthreads();
    uint16_t nj[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * CS_PNG_THREADS;
      nj[k] = i <= n ? jump[jump[i]] : (uint16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * CS_PNG_THREADS;
      if (i <= n) jump[i] = nj[k];
    }
    __syncthreads();
  }
  // ---- d. the chunk image: [length][IDAT][78 01 when first][deflate ...][crc]
  for (int w = tid; w < kOutWords; w += CS_PNG_THREADS) out32[w] = 0;
  __syncthreads();
  const int pay0 = 8 + (first ? 2 : 0);             // byte offset of the deflate data in the chunk image
  const int stored_bytes = 5 + n;
  int plen;  // chunk data bytes
  if constexpr ((FLAGS & 1) == 0) {
    uint32_t bitpos = (uint32_t)pay0 * 8u + 3u;       // running bit offset; 3 header bits first
    for (int base = 0; base < n; base += CS_PNG_THREADS) {
      const int i = base + tid;
      uint2 tb = make_uint2(0u, 0u);
      if (i < n) {
        const uint32_t e = ld[i];
        if (e & 0x80000000u) tb = token_bits(in8[i], (int)(e & 0x1ffu), (int)((e >> 9) & 0x3fffu));
      }
      uint32_t inc = tb.y;  // inclusive wave scan
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      if (lane == 63) red[wv] = inc;
      __syncthreads();
      uint32_t before = 0, all = 0;
      for (int k = 0; k < NW; ++k) { const uint32_t u = red[k]; if (k < wv) before += u; all += u; }
      const uint32_t o = bitpos + before + inc - tb.y;
      if (tb.y && (int)(o >> 5) + 1 < kOutWords) {
        const uint64_t v = (uint64_t)tb.x << (o & 31u);
        atomicOr(&out32[o >> 5], (uint32_t)v);
        if ((uint32_t)(v >> 32)) atomicOr(&out32[(o >> 5) + 1], (uint32_t)(v >> 32));
      }
      bitpos += all;
      __syncthreads();
    }
    // end-of-block (7 zero bits), then either BFINAL's padding or the empty stored block 000 | pad | 00 00 FF FF
    const uint32_t endbits = bitpos + 7u + (last ? 0u : 3u);
    const int fixed_bytes = (int)((endbits + 7u) / 8u) - pay0 + (last ? 0 : 4);
    const bool use_fixed = fixed_bytes < stored_bytes;
    if (use_fixed) {
      plen = (first ? 2 : 0) + fixed_bytes;
      if (tid == 0) {
        atomicOr(&out32[(pay0 * 8) >> 5], (uint32_t)((last ? 1u : 0u) | 2u) << ((pay0 * 8) & 31));  // BFINAL, BTYPE = 01
        if (!last) { out8[8 + plen - 2] = 0xff; out8[8 + plen - 1] = 0xff; }
      }
    } else {
      plen = (first ? 2 : 0) + stored_bytes;
      for (int w = tid; w < kOutWords; w += CS_PNG_THREADS) out32[w] = 0;
      __syncthreads();
      if (tid == 0) {
        out8[pay0] = last ? 1 : 0;
        out8[pay0 + 1] = (uint8_t)(n & 0xff); out8[pay0 + 2] = (uint8_t)(n >> 8);
        out8[pay0 + 3] = (uint8_t)(~n & 0xff); out8[pay0 + 4] = (uint8_t)((~n >> 8) & 0xff);
      }
      for (int t = tid; t < n; t += CS_PNG_THREADS) out8[pay0 + 5 + t] = in8[t];
    }
  } else {
    using namespace cs_huff;
    DynLds& D = *reinterpret_cast<DynLds*>(png_lds + kLdsBytes);
    // d1. counts of both forms, each with one end-of-block; the fixed set's lengths
    for (int t = tid; t < 2 * kAlpha; t += CS_PNG_THREADS) (&D.hist[0][0])[t] = 0;
    for (int t = tid; t < 3 * kAlpha; t += CS_PNG_THREADS) (&D.len[0][0])[t] = t >= 2 * kAlpha ? (uint8_t)fixed_length(t - 2 * kAlpha) : (uint8_t)0;
    if (tid < 3) D.bits[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += CS_PNG_THREADS) {
      const uint32_t byte = in8[i], e = ld[i];
      atomicAdd(&D.hist[1][byte], 1u);
      if (e & 0x80000000u) {
        const int l = (int)(e & 0x1ffu);
        if (l < 3) atomicAdd(&D.hist[0][byte], 1u);
        else {
          uint32_t sy, eb, ev, dc, db, dv;
          length_symbol(l, &sy, &eb, &ev);
          dist_symbol((int)((e >> 9) & 0x3fffu), &dc, &db, &dv);
          atomicAdd(&D.hist[0][sy], 1u);
          atomicAdd(&D.hist[0][kLL + dc], 1u);
        }
      }
    }
    if (tid == 0) { atomicAdd(&D.hist[0][256], 1u); atomicAdd(&D.hist[1][256], 1u); }
    __syncthreads();
    // d2. the used symbols of each tree in ascending (count, symbol) order: every symbol finds its own rank
    for (int w = tid; w < kAlpha + kLL; w += CS_PNG_THREADS) {
      const int tree = w < kLL ? 0 : w < kAlpha ? 1 : 2;
      const uint32_t* h = D.hist[tree == 2 ? 1 : 0];
      const int t = tree == 2 ? w - kAlpha : w, lo = tree == 1 ? kLL : 0, hi = tree == 1 ? kAlpha : kLL;
      if (h[t] || t == lo) {
        int used;
        const int r = sort_rank(h, lo, hi, t, &used);
        if (h[t]) { D.key[tree][r] = h[t]; D.sym[tree][r] = (uint16_t)t; }
        if (t == lo) D.used[tree] = (uint32_t)used;
      }
    }
    __syncthreads();
    // d3. code lengths, codes and block header: one lane per set, serial over symbols
    if (tid == 0 || tid == 64) {
      const int s = tid >> 6;
      code_lengths(D.key[2 * s], D.sym[2 * s], (int)D.used[2 * s], 0, 15, D.num[s], D.len[s]);
      if (s == 0) code_lengths(D.key[1], D.sym[1], (int)D.used[1], kLL, 15, D.num[s], D.len[s]);
      canonical_codes(D.len[s], kLL, 15, D.num[s], D.code[s]);
      canonical_codes(D.len[s] + kLL, kD, 15, D.num[s], D.code[s] + kLL);
      D.hdrbits[s] = dynamic_header(D.len[s], &D.hs[s], D.hdr[s]);
    } else if (tid == 128) {
      canonical_codes(D.len[2], kLL, 15, D.num[2], D.code[2]);
      canonical_codes(D.len[2] + kLL, kD, 15, D.num[2], D.code[2] + kLL);
    }
    __syncthreads();
    // d4. exact sizes from the counts; the smallest form wins, a later one only when strictly smaller in bytes
    if (tid < kAlpha) {
      const uint32_t h0 = D.hist[0][tid], h1 = D.hist[1][tid], x = extra_bits(tid);
      if (h0) { atomicAdd(&D.bits[0], h0 * (D.len[0][tid] + x)); atomicAdd(&D.bits[2], h0 * (fixed_length(tid) + x)); }
      if (h1) atomicAdd(&D.bits[1], h1 * D.len[1][tid]);
    }
    __syncthreads();
    auto block_bytes = [&](uint32_t bits) { return (int)(last ? (3u + bits + 7u) / 8u : (3u + bits + 3u + 7u) / 8u + 4u); };
    int choice = 0, best_bytes = stored_bytes;  // 0 stored, 1 fixed + tokens, 2 dynamic + tokens, 3 dynamic + literals
    { const int c = block_bytes(D.bits[2]); if (c < best_bytes) { best_bytes = c; choice = 1; } }
    { const int c = block_bytes(D.hdrbits[0] + D.bits[0]); if (c < best_bytes) { best_bytes = c; choice = 2; } }
    { const int c = block_bytes(D.hdrbits[1] + D.bits[1]); if (c < best_bytes) { best_bytes = c; choice = 3; } }
    if (choice != 0) {
      // d5. the winner's bits: header words, then a token per reached position (or a literal per byte), then end-of-block
      const int set = choice == 1 ? 2 : choice == 2 ? 0 : 1;
      const bool literals = choice == 3;
      const uint16_t* code = D.code[set];
      const uint8_t* len = D.len[set];
      uint32_t bitpos = (uint32_t)pay0 * 8u + 3u;
      if (choice >= 2) {
        const uint32_t hb = D.hdrbits[set];
        if (tid < kHdrWords && (uint32_t)tid * 32u < hb) {
          const uint32_t o = bitpos + 32u * (uint32_t)tid;
          const uint64_t v = (uint64_t)D.hdr[set][tid] << (o & 31u);
          if ((int)(o >> 5) + 1 < kOutWords) {
            if ((uint32_t)v) atomicOr(&out32[o >> 5], (uint32_t)v);
            if ((uint32_t)(v >> 32)) atomicOr(&out32[(o >> 5) + 1], (uint32_t)(v >> 32));
          }
        }
        bitpos += hb;
      }
      for (int base = 0; base < n; base += CS_PNG_THREADS) {
        const int i = base + tid;
        uint64_t v = 0;   // a dynamic-coded match is up to 15 + 5 + 15 + 13 = 48 bits
        uint32_t nb = 0;
        if (i < n) {
          const uint32_t e = ld[i], byte = in8[i];
          const int l = (int)(e & 0x1ffu);
          if (literals || ((e & 0x80000000u) && l < 3)) { v = code[byte]; nb = len[byte]; }
          else if (e & 0x80000000u) {
            uint32_t sy, eb, ev, dc, db, dv;
            length_symbol(l, &sy, &eb, &ev);
            dist_symbol((int)((e >> 9) & 0x3fffu), &dc, &db, &dv);
            v = code[sy]; nb = len[sy];
            v |= (uint64_t)ev << nb; nb += eb;
            v |= (uint64_t)code[kLL + dc] << nb; nb += len[kLL + dc];
            v |= (uint64_t)dv << nb; nb += db;
          }
        }
        uint32_t inc = nb;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t u = __shfl_up(inc, o, 64);
          if (lane >= o) inc += u;
        }
        if (lane == 63) red[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < NW; ++k) { const uint32_t u = red[k]; if (k < wv) before += u; all += u; }
        const uint32_t o = bitpos + before + inc - nb;
        if (nb && (int)(o >> 5) + 2 < kOutWords) {  // up to three words
          const uint32_t sh = o & 31u;
          const uint64_t lo = v << sh;
          const uint32_t hi = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
          if ((uint32_t)lo) atomicOr(&out32[o >> 5], (uint32_t)lo);
          if ((uint32_t)(lo >> 32)) atomicOr(&out32[(o >> 5) + 1], (uint32_t)(lo >> 32));
          if (hi) atomicOr(&out32[(o >> 5) + 2], hi);
        }
        bitpos += all;
        __syncthreads();
      }
      const uint32_t endbits = bitpos + len[256] + (last ? 0u : 3u);
      // equals the priced size, which is below the stored form's; the min keeps the chunk inside its staging slot whatever happens
      const int block = min((int)((endbits + 7u) / 8u) - pay0 + (last ? 0 : 4), stored_bytes);
      plen = (first ? 2 : 0) + block;
      if (tid == 0) {
        if ((int)(bitpos >> 5) + 1 < kOutWords) {
          const uint64_t v = (uint64_t)code[256] << (bitpos & 31u);
          atomicOr(&out32[bitpos >> 5], (uint32_t)v);
          if ((uint32_t)(v >> 32)) atomicOr(&out32[(bitpos >> 5) + 1], (uint32_t)(v >> 32));
        }
        atomicOr(&out32[(pay0 * 8) >> 5], (uint32_t)((last ? 1u : 0u) | (choice == 1 ? 2u : 4u)) << ((pay0 * 8) & 31));  // BFINAL, BTYPE = 01 / 10
        if (!last) { out8[8 + plen - 2] = 0xff; out8[8 + plen - 1] = 0xff; }
      }
    } else {
      plen = (first ? 2 : 0) + stored_bytes;
      if (tid == 0) {
        out8[pay0] = last ? 1 : 0;
        out8[pay0 + 1] = (uint8_t)(n & 0xff); out8[pay0 + 2] = (uint8_t)(n >> 8);
        out8[pay0 + 3] = (uint8_t)(~n & 0xff); out8[pay0 + 4] = (uint8_t)((~n >> 8) & 0xff);
      }
      for (int t = tid; t < n; t += CS_PNG_THREADS) out8[pay0 + 5 + t] = in8[t];
    }
  }
  __syncthreads();
  if (tid == 0) {
    out8[0] = (uint8_t)(plen >> 24); out8[1] = (uint8_t)(plen >> 16); out8[2] = (uint8_t)(plen >> 8); out8[3] = (uint8_t)plen;
    out8[4] = 'I'; out8[5] = 'D'; out8[6] = 'A'; out8[7] = 'T';
    if (first) { out8[8] = 0x78; out8[9] = 0x01; }
  }
  __syncthreads();
  // ---- e. CRC-32 over type + data = out8[4 .. 8 + plen)
  const int L = 4 + plen;
  const int nsl = (L + 35) / 36;
  uint32_t acc = 0;
  for (int j = tid; j < nsl; j += CS_PNG_THREADS) {
    const int b0 = j * 36, b1 = min(L, b0 + 36);
    uint32_t c = j == 0 ? 0xffffffffu : 0u;
    for (int w = b0; w < b1; w += 4) {
      uint32_t word = out32[1 + (w >> 2)];
      const int nb = min(4, b1 - w);
      for (int e = 0; e < nb; ++e) { c = crct[(c ^ word) & 0xffu] ^ (c >> 8); word >>= 8; }
    }
    int behind = L - b1;
    for (int k = 0; behind; ++k, behind >>= 1)
      if (behind & 1) c = crc_mulmod(c, cpow[k]);
    acc ^= c;
  }
  acc = wave_xor(acc);
  if (lane == 0) red[32 + wv] = acc;
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
    for (int k = 0; k < NW; ++k) c ^= red[32 + k];
    c ^= 0xffffffffu;
    out8[8 + plen] = (uint8_t)(c >> 24); out8[8 + plen + 1] = (uint8_t)(c >> 16); out8[8 + plen + 2] = (uint8_t)(c >> 8); out8[8 + plen + 3] = (uint8_t)c;
  }
  __syncthreads();
  // ---- f. staging: record (chunk bytes, S, T, 0), then the chunk
  uint32_t* slot = reinterpret_cast<uint32_t*>(staging + ((size_t)img * g.nseg + seg) * CS_PNG_SLOT);
  const int cwords = (12 + plen + 3) / 4;
  if (tid == 0) { slot[0] = 12u + (uint32_t)plen; slot[1] = adler_s; slot[2] = adler_t; slot[3] = 0u; }
  for (int w = tid; w < cwords; w += CS_PNG_THREADS) slot[4 + w] = out32[w];
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

__device__ uint32_t crc_bytes_serial(const uint8_t* p, int n) {  // the fixed-size chunks only (IHDR 17 bytes, Adler 8)
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  }
  return c ^ 0xffffffffu;
}

__global__ __launch_bounds__(256) void png_assemble_kernel(const uint8_t* __restrict__ staging, PngGeom g, uint8_t* __restrict__ out, size_t slot_bytes,
                                                           uint32_t* __restrict__ lengths) {
  __shared__ unsigned long long red[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int seg = blockIdx.x, img = blockIdx.y;
  const bool last = seg == g.nseg - 1;
  const uint8_t* stg = staging + (size_t)img * g.nseg * CS_PNG_SLOT;
  // offset of this chunk = bytes of the chunks before it; the last segment's workgroup also combines the Adler sums of all segments:
  // s1 = 1 + sum S_k, s2 = total + sum (T_k + S_k * bytes behind segment k)   (mod 65521)
  unsigned long long off = 0, s1 = 0, s2 = 0;
  const int upto = last ? g.nseg : seg;
  for (int k = tid; k < upto; k += 256) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(stg + (size_t)k * CS_PNG_SLOT);
    if (k < seg) off += rec[0];
    if (last) {
      const unsigned long long end = min((unsigned long long)(k + 1) * CS_PNG_SEG, (unsigned long long)g.total);
      s1 += rec[1];
      s2 += (rec[2] + (unsigned long long)rec[1] * ((g.total - end) % kAdlerMod)) % kAdlerMod;
    }
  }
  for (int o = 32; o >= 1; o >>= 1) { off += __shfl_xor(off, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  if (lane == 0) { red[0][wv] = off; red[1][wv] = s1; red[2][wv] = s2; }
  __syncthreads();
  off = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  uint8_t* file = out + (size_t)img * slot_bytes;
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(stg + (size_t)seg * CS_PNG_SLOT);
  const int cbytes = (int)rec[0];
  const uint32_t* s32 = rec + 4;
  uint8_t* dst = file + 33 + off;
  // A file that does not fit its slot (impossible while slot_bytes >= cs_png_bound, which the host checks) fails loudly: no workgroup writes
  // past the slot, and the file's length becomes 0.  Chunk ends grow with the segment index (off_last + c_last >= off_k + c_k for every k),
  // so whenever any chunk of the image trips this test the last one does too, and the last segment's workgroup is the only writer of
  // lengths[img]: the length is 0 or that of a complete file, never that of a file with a hole.  PngHandle raises on a zero length.
  if (33 + off + (unsigned long long)cbytes + 28 > slot_bytes) {
    if (last && tid == 0) lengths[img] = 0;
    return;
  }
  // word copy onto the destination's alignment
  const int head = min(cbytes, (int)((4 - ((uintptr_t)dst & 3)) & 3));
  const int nw = (cbytes - head) / 4;
  const uint8_t* s8 = reinterpret_cast<const uint8_t*>(s32);
  if (tid < head) dst[tid] = s8[tid];
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
  for (int w = tid; w < nw; w += 256) d32[w] = ld32(s32, head + 4 * w);
  const int tail0 = head + 4 * nw;
  if (tid < cbytes - tail0) dst[tail0 + tid] = s8[tail0 + tid];
  if (seg == 0 && tid == 0) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) file[i] = sig[i];
    uint8_t* h = file + 8;
    put_be32(h, 13u);
    h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
    put_be32(h + 8, (uint32_t)g.W);
    put_be32(h + 12, (uint32_t)g.H);
    h[16] = g.kind == 0 ? 16 : 8;  // bit depth
    h[17] = g.kind == 0 ? 0 : 2;   // colour type: gray / truecolour
    h[18] = 0; h[19] = 0; h[20] = 0;  // deflate, adaptive filtering, no interlace
    uint8_t tmp[17];
    for (int i = 0; i < 17; ++i) tmp[i] = h[4 + i];
    put_be32(h + 21, crc_bytes_serial(tmp, 17));
  }
  if (last && tid == 0) {
    const unsigned long long S1 = (1ull + red[1][0] + red[1][1] + red[1][2] + red[1][3]) % kAdlerMod;
    const unsigned long long S2 = ((unsigned long long)g.total % kAdlerMod + red[2][0] + red[2][1] + red[2][2] + red[2][3]) % kAdlerMod;
    uint8_t tmp[8] = {'I', 'D', 'A', 'T', 0, 0, 0, 0};
    put_be32(tmp + 4, (uint32_t)((S2 << 16) | S1));
    uint8_t* a = dst + cbytes;
    put_be32(a, 4u);
    for (int i = 0; i < 8; ++i) a[4 + i] = tmp[i];
    put_be32(a + 12, crc_bytes_serial(tmp, 8));
    uint8_t* e = a + 16;
    put_be32(e, 0u);
    e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
    put_be32(e + 8, 0xAE426082u);
    lengths[img] = (uint32_t)(33 + off + cbytes + 16 + 12);
  }
}

// de_norm_img + u8 (utils/misc/image.py:25-34, utils/io/images.py:20-23): fp32 CHW -> uint8 HWC; x * std, + mean, * 255, each rounded on its
// own (no fma contraction), truncated; clamped to [0, 255] (NaN -> 0)
__global__ __launch_bounds__(256) void denorm_rgb8_kernel(const float* __restrict__ chw, long long hw, long long total, float m0, float m1, float m2,
                                                          float s0, float s1, float s2, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)  // the host form rounds the product before the sum: no fma here
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // pixel over all images
  if (i >= total) return;
  const long long im = i / hw, p = i - im * hw;
  const float* x = chw + im * 3 * hw + p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = x[c * hw] * sd[c];
    v = v + mean[c];
    v = v * 255.0f;
    v = v >= 0.f ? v : 0.f;  // NaN -> 0
    v = v <= 255.f ? v : 255.f;
    out[i * 3 + c] = (uint8_t)(int)v;
  }
}

bool png_geom(int kind, int H, int W, PngGeom* g) {
  if ((kind != 0 && kind != 1) || H <= 0 || W <= 0) return false;
  g->kind = kind; g->H = H; g->W = W;
  g->bpp = kind == 0 ? 2 : 3;
  g->rb = W * g->bpp;
  g->rl = 1 + g->rb;
  const unsigned long long total = (unsigned long long)H * g->rl;
  g->total = (unsigned)total;
  g->nseg = (int)((total + CS_PNG_SEG - 1) / CS_PNG_SEG);
  return true;
}

template <int FLAGS>
hipError_t png_launch_segments(const uint8_t* pixels, long long image_stride, const PngGeom& g, int I, uint8_t* staging, hipStream_t st) {
  constexpr int lds = kLdsBytes + ((FLAGS & 1) ? (int)sizeof(DynLds) : 0);
  // more than 64 KiB of dynamic LDS needs the attribute on the current device; set on every call (a host-side table write, no device work)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(png_segment_kernel<FLAGS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(png_segment_kernel<FLAGS>, dim3(g.nseg, I), dim3(CS_PNG_THREADS), lds, st, pixels, image_stride, g, staging);
  return hipGetLastError();
}

}  // namespace

extern "C" {

// 4096 x 4096 RGB: 50 335 744 filtered bytes, 3073 segments
int cs_png_size_supported(int H, int W) { return H <= CS_PNG_MAX_SIDE && W <= CS_PNG_MAX_SIDE; }

size_t cs_png_bound_bytes(int kind, int H, int W) {
  PngGeom g;
  if (!png_geom(kind, H, W, &g)) return 0;
  // per segment: chunk framing 12 + stored-block header 5; the zlib header 2; the fixed parts
  return (size_t)g.total + (size_t)g.nseg * 17 + 2 + CS_PNG_FIXED;
}

size_t cs_png_staging_bytes(int kind, int I, int H, int W) {
  PngGeom g;
  if (I <= 0 || !png_geom(kind, H, W, &g)) return 0;
  return (size_t)I * g.nseg * CS_PNG_SLOT;
}

hipError_t cs_png_encode_launch(const void* pixels, int kind, int I, int H, int W, long long image_stride, uint8_t* out, size_t slot_bytes,
                                uint32_t* lengths, void* workspace, int flags, hipStream_t st) {
  PngGeom g;
  if (!png_geom(kind, H, W, &g) || I <= 0 || I > 65535 || flags < 0 || flags > 3) return hipErrorInvalidValue;
  const uint8_t* px = (const uint8_t*)pixels;
  uint8_t* stg = (uint8_t*)workspace;
  hipError_t e = flags == 0   ? png_launch_segments<0>(px, image_stride, g, I, stg, st)
                 : flags == 1 ? png_launch_segments<1>(px, image_stride, g, I, stg, st)
                 : flags == 2 ? png_launch_segments<2>(px, image_stride, g, I, stg, st)
                              : png_launch_segments<3>(px, image_stride, g, I, stg, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(png_assemble_kernel, dim3(g.nseg, I), dim3(256), 0, st, (const uint8_t*)workspace, g, out, slot_bytes, lengths);
  return hipGetLastError();
}

hipError_t cs_denorm_rgb8_launch(const float* chw, int I, int H, int W, const float* mean3, const float* std3, uint8_t* out, hipStream_t st) {
  const long long hw = (long long)H * W, total = hw * I;
  hipLaunchKernelGGL(denorm_rgb8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, chw, hw, total, mean3[0], mean3[1], mean3[2], std3[0],
                     std3[1], std3[2], out);
  return hipGetLastError();
}

}  // extern "C"
