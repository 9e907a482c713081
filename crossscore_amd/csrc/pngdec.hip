// PNG decoder on the device (gfx950): compressed files in, uint8 HWC / uint16 images out.  The mirror of png.hip.
//
// One workgroup of one wave decodes one file, start to end; the rate comes from the files of a call being in flight together.
//   1. framing      signature, IHDR (size and format against the call's), every IDAT span against the file's length
//   2. CRC + gather  CRC-32 of IHDR and of every IDAT chunk (lanes take slices through a 256-entry table in LDS, the slices' remainders are
//                    multiplied by x^(8 * bytes behind them) mod P and XOR-reduced, as png.hip does it); the same pass copies the IDAT payloads
//                    into the file's slice of the workspace, so that the zlib stream is contiguous wherever the chunks were split
//   3. inflate      one serial symbol loop whose state (bit buffer, positions) is wave-uniform and lives in scalar registers; the stream is
//                    staged through LDS 1 KiB at a time; decode tables are built in LDS per block (10-bit primary lookup, canonical-code walk
//                    for longer codes); literals go into a 32-KiB ring in LDS, matches are copied inside the ring by all lanes (an overlapping
//                    copy reads the period it repeats), and the ring is flushed to the workspace 16 KiB at a time by all lanes, which also
//                    accumulate the Adler-32 of what they flush.  Back-references never read global memory.
//   4. un-filter    lane l takes row r0 + l of a band of 64 rows and is one pixel behind lane l - 1, so the pixel above and above-left arrive
//                    through a lane shift (the row above a band's first row waits in LDS); all five filter types, 1-4 bytes per pixel, with
//                    the alpha drop, the gray replication and the big-endian -> native swap in the store.
// A file that fails any check ends its workgroup with a status word and writes no pixel.
//
// Untrusted input: every read of the file is at an index below its length (the spans are re-checked here against the length, whatever the
// host's probe said); the stream reader hands out zeros past the end of the gathered stream and raises "input exhausted"; every write to the
// workspace is below the expected stream length H * (1 + row bytes), which the slot holds; pixels are written for r < H, x < W only.
#include "cs_common.h"

#define CS_PNGDEC_THREADS 64
#define CS_PNGDEC_RING 32768
#define CS_PNGDEC_FLUSH 16384
#define CS_PNGDEC_IN_WORDS 256
#define CS_PNGDEC_PB 10  // bits of the primary lookup

namespace {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kAdlerMod = 65521u;

// status words (include/crossscore_hip.h: CS_PNGDEC_*)
enum {
  ST_OK = 0, ST_CRC = 1, ST_ADLER = 2, ST_ZLIB_HEADER = 3, ST_BLOCK_TYPE = 4, ST_STORED_LEN = 5, ST_BAD_CODE = 6, ST_BAD_SYMBOL = 7,
  ST_DISTANCE = 8, ST_SHORT = 9, ST_LONG = 10, ST_FILTER = 11, ST_EXHAUSTED = 12, ST_HEADER = 13, ST_FRAMING = 14
};

struct PngDecArgs {
  const uint8_t* files;
  const unsigned long long* file_offsets;
  const uint32_t* file_lengths;
  const uint32_t* spans;  // (offset, length) pairs, offsets relative to the file
  const uint32_t* span_offsets;  // I + 1 entries
  unsigned long long files_bytes;
  int kind, H, W;
  uint8_t* pixels;
  long long image_stride;
  uint32_t* status;
  uint8_t* filtered;  // workspace: I slots of fslot bytes
  unsigned long long fslot;
  uint8_t* streams;  // workspace: the gathered zlib streams
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

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

__device__ __forceinline__ uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// LDS of the kernel
struct PngDecLds {
  uint8_t ring[CS_PNGDEC_RING];  // the last 32 KiB of output; the un-filter's row buffer afterwards
  uint16_t ltab[1 << CS_PNGDEC_PB];  // literal/length primary table: symbol | length << 9, 0 = walk the canonical code
  uint16_t dtab[1 << CS_PNGDEC_PB];  // distance primary table (the code-length code's while a dynamic header is read)
  uint16_t lsyms[288], dsyms[32];    // symbols ordered by (code length, symbol)
  uint16_t lcnt[16], lfirst[16], lstart[16], dcnt[16], dfirst[16], dstart[16];  // per code length: symbols, first code, index of its first symbol
  uint16_t cur[16];  // build_table's per-length cursors
  uint8_t lens[384];  // code lengths: the fixed code's 288 + 32, or the code-length code's 19 and, from 32 on, a dynamic block's <= 316
  uint32_t crct[256];
  uint32_t cpow[28];  // x^(8 * 2^j)
  uint32_t inw[CS_PNGDEC_IN_WORDS];
  unsigned long long red[2];
  int err;
};

// CRC-32 of file[start, start + L) by all lanes; bytes from index `skip` on are also copied to dst (the chunk's payload behind its type)
__device__ __forceinline__ uint32_t region_crc(const PngDecLds& s, const uint8_t* file, uint32_t start, uint32_t L, uint8_t* dst, uint32_t skip, int lane) {
  const uint32_t per = (L + 63u) / 64u;
  const uint32_t b0 = min(L, (uint32_t)lane * per), b1 = min(L, b0 + per);
  uint32_t c = lane == 0 ? 0xffffffffu : 0u;
  for (uint32_t i = b0; i < b1; ++i) {
    const uint32_t b = file[start + i];
    if (dst && i >= skip) dst[i - skip] = (uint8_t)b;
    c = s.crct[(c ^ b) & 0xffu] ^ (c >> 8);
  }
  uint32_t behind = L - b1;
  for (int k = 0; behind; ++k, behind >>= 1)
    if (behind & 1u) c = crc_mulmod(c, s.cpow[k]);
  return wave_xor(c) ^ 0xffffffffu;
}

// The bit reader: wave-uniform state.  bb holds nb valid bits (LSB first); iw is the next word of the stream to take.
struct Bits {
  unsigned long long bb;
  int nb;
  uint32_t iw, ibase;
  uint32_t nbytes, nwords;
  const uint32_t* words;  // the gathered stream, 4-byte aligned, zero bytes behind its end up to the word
};

__device__ __forceinline__ void load_input(PngDecLds& s, Bits& r, int lane) {
  __syncthreads();
  r.ibase = r.iw;
#pragma unroll
  for (int k = 0; k < CS_PNGDEC_IN_WORDS / 64; ++k) {
    const uint32_t idx = r.ibase + (uint32_t)lane + 64u * k;
    s.inw[lane + 64 * k] = idx < r.nwords ? r.words[idx] : 0u;  // zeros past the end
  }
  __syncthreads();
}

// at least 32 valid bits afterwards
__device__ __forceinline__ void refill(PngDecLds& s, Bits& r, int lane) {
  if (r.nb <= 32) {
    if (r.iw - r.ibase >= CS_PNGDEC_IN_WORDS) load_input(s, r, lane);
    const uint32_t w = rfl(s.inw[r.iw - r.ibase]);
    r.bb |= (unsigned long long)w << r.nb;
    r.nb += 32;
    r.iw += 1;
  }
}

__device__ __forceinline__ uint32_t take(Bits& r, int n) {  // n <= 32 bits that refill() has made available
  const uint32_t v = (uint32_t)(r.bb & ((1ull << n) - 1ull));
  r.bb >>= n;
  r.nb -= n;
  return v;
}

__device__ __forceinline__ unsigned long long consumed_bits(const Bits& r) { return (unsigned long long)r.iw * 32ull - (unsigned long long)r.nb; }
__device__ __forceinline__ bool exhausted(const Bits& r) { return consumed_bits(r) > (unsigned long long)r.nbytes * 8ull; }

__device__ __forceinline__ void seek_byte(PngDecLds& s, Bits& r, uint32_t bytepos, int lane) {
  r.iw = bytepos >> 2;
  r.bb = 0;
  r.nb = 0;
  load_input(s, r, lane);
  refill(s, r, lane);
  take(r, (int)(bytepos & 3u) * 8);
}

// Canonical Huffman tables of n code lengths in LDS.  Returns 0 or ST_BAD_CODE (over-subscribed; incomplete unless the longest code is one bit,
// which is zlib's rule, and never for the code-length code).
__device__ __forceinline__ int build_table(PngDecLds& s, const uint8_t* lens, int n, uint16_t* tab, int pb, uint16_t* cnt, uint16_t* first, uint16_t* start, uint16_t* syms,
                           bool strict, int lane) {
  __syncthreads();
  if (lane == 0) {
    int e = 0;
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i]] += 1;
    int left = 1, maxl = 0;
    for (int l = 1; l < 16; ++l) {
      left = (left << 1) - (int)cnt[l];
      if (left < 0) { e = ST_BAD_CODE; break; }
      if (cnt[l]) maxl = l;
    }
    if (!e && left > 0 && (int)cnt[0] != n && (strict || maxl != 1)) e = ST_BAD_CODE;
    uint16_t off = 0, code = 0, prev = 0;
    for (int l = 1; l < 16; ++l) {
      code = (uint16_t)((code + prev) << 1);
      prev = cnt[l];
      first[l] = code;
      start[l] = off;
      off += cnt[l];
    }
    first[0] = 0;
    start[0] = 0;
    if (!e) {
      for (int l = 0; l < 16; ++l) s.cur[l] = start[l];
      for (int i = 0; i < n; ++i) {
        const int l = lens[i];
        if (l) { syms[s.cur[l]] = (uint16_t)i; s.cur[l] += 1; }
      }
    }
    s.err = e;
  }
  for (int k = lane; k < (1 << pb); k += 64) tab[k] = 0;
  __syncthreads();
  const int e = (int)rfl((uint32_t)s.err);
  if (e) return e;
  const int used = n - (int)cnt[0];
  for (int j = lane; j < used; j += 64) {
    const uint32_t sym = syms[j];
    const int l = lens[sym];
    if (l <= pb) {
      const uint32_t code = (uint32_t)first[l] + (uint32_t)(j - (int)start[l]);
      const uint32_t rev = __brev(code) >> (32 - l);
      for (uint32_t k = rev; k < (1u << pb); k += 1u << l) tab[k] = (uint16_t)(sym | ((uint32_t)l << 9));
    }
  }
  __syncthreads();
  return 0;
}

// one symbol: the primary lookup, else the canonical walk.  Returns the symbol or -1 (no code of the set matches the bits).
__device__ __forceinline__ int decode_sym(Bits& r, const uint16_t* tab, int pb, const uint16_t* cnt, const uint16_t* first, const uint16_t* start,
                                          const uint16_t* syms) {
  const uint32_t e = rfl(tab[(uint32_t)r.bb & ((1u << pb) - 1u)]);
  if (e) {
    take(r, (int)(e >> 9));
    return (int)(e & 511u);
  }
  const uint32_t rev = __brev((uint32_t)r.bb);  // stream order, first bit at bit 31
  for (int l = 1; l < 16; ++l) {
    const uint32_t code = rev >> (32 - l);
    const uint32_t f = rfl(first[l]), c = rfl(cnt[l]);
    if (code >= f && code - f < c) {
      take(r, l);
      return (int)rfl(syms[rfl(start[l]) + (code - f)]);
    }
  }
  return -1;
}

// ring[flushed, flushed + n) -> the filtered stream, with its Adler sums: A += S, B += n * A + T
__device__ __forceinline__ void flush_ring(PngDecLds& s, uint8_t* out, uint32_t flushed, uint32_t n, uint32_t& adA, uint32_t& adB, int lane) {
  __syncthreads();
  uint32_t S = 0;
  unsigned long long T = 0;
  if ((n & 1023u) == 0 && (flushed & 15u) == 0) {
    for (uint32_t base = 0; base < n; base += 1024u) {
      const uint32_t i0 = base + (uint32_t)lane * 16u;
      const uint4 v = *reinterpret_cast<const uint4*>(&s.ring[(flushed + i0) & (CS_PNGDEC_RING - 1)]);
      *reinterpret_cast<uint4*>(out + flushed + i0) = v;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t b = (w[q] >> (8 * e)) & 0xffu;
          S += b;
          T += (unsigned long long)(n - (i0 + 4 * q + e)) * b;
        }
    }
  } else {
    for (uint32_t i = lane; i < n; i += 64u) {
      const uint32_t b = s.ring[(flushed + i) & (CS_PNGDEC_RING - 1)];
      out[flushed + i] = (uint8_t)b;
      S += b;
      T += (unsigned long long)(n - i) * b;
    }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    S += __shfl_xor(S, o, 64);
    T += __shfl_xor(T, o, 64);
  }
  S = rfl(S);
  const uint32_t Tm = rfl((uint32_t)(T % kAdlerMod));
  adB = (uint32_t)((adB + (unsigned long long)(n % kAdlerMod) * adA + Tm) % kAdlerMod);
  adA = (adA + S % kAdlerMod) % kAdlerMod;
  __syncthreads();
}

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ __launch_bounds__(CS_PNGDEC_THREADS) void png_decode_kernel(PngDecArgs a) {
  __shared__ __attribute__((aligned(16))) PngDecLds s;
  const int lane = threadIdx.x;
  const int img = blockIdx.x;
  int st = ST_OK;

  // ---- tables
  for (int i = lane; i < 256; i += 64) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    s.crct[i] = c;
  }
  if (lane < 28) {
    uint32_t p = 0x40000000u;  // x^1
    for (int k = 0; k < lane + 3; ++k) p = crc_mulmod(p, p);
    s.cpow[lane] = p;
  }
  if (lane == 0) s.err = 0;
  __syncthreads();

  // ---- 1. framing
  const unsigned long long foff = a.file_offsets[img];
  const uint32_t flen = a.file_lengths[img];
  const uint32_t sp0 = a.span_offsets[img], sp1 = a.span_offsets[img + 1];
  const uint8_t* file = a.files + foff;
  int bpp = 0;  // bytes per pixel of the file
  if (flen < 57u || flen >= (1u << 28) || foff > a.files_bytes || (unsigned long long)flen > a.files_bytes - foff || sp1 <= sp0) {
    st = ST_FRAMING;
  } else {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) ok = ok && file[i] == sig[i];
    ok = ok && be32(file + 8) == 13u && be32(file + 12) == 0x49484452u;  // "IHDR"
    if (!ok) st = ST_FRAMING;
    else {
      const uint32_t w = be32(file + 16), h = be32(file + 20);
      const int depth = file[24], ct = file[25];
      if (a.kind == 1) bpp = (depth == 8 && ct == 2) ? 3 : (depth == 8 && ct == 6) ? 4 : (depth == 8 && ct == 0) ? 1 : 0;
      else bpp = (depth == 16 && ct == 0) ? 2 : 0;
      if (w != (uint32_t)a.W || h != (uint32_t)a.H || bpp == 0 || file[26] != 0 || file[27] != 0 || file[28] != 0) st = ST_HEADER;
    }
  }
  st = (int)rfl((uint32_t)st);
  bpp = (int)rfl((uint32_t)bpp);
  const uint32_t rb = (uint32_t)a.W * (uint32_t)bpp;  // row bytes of the file
  const uint32_t pitch = rb + 1u;
  const uint32_t total = (uint32_t)a.H * pitch;  // <= 4096 * (4 * 4096 + 1)
  uint8_t* fil = a.filtered + (unsigned long long)img * a.fslot;
  // the file's slice of the stream area: 4-byte aligned, flen + 4 bytes at least (the next file's starts 8 bytes further than its offset says)
  uint8_t* stream = a.streams + ((foff + 8ull * (unsigned)img + 3ull) & ~3ull);
  uint32_t nstream = 0;

  // ---- 2. CRCs, and the IDAT payloads gathered into one stream
  if (!st) {
    if (region_crc(s, file, 12u, 17u, nullptr, 0u, lane) != be32(file + 29)) st = ST_CRC;
    for (uint32_t k = sp0; k < sp1 && !st; ++k) {
      const uint32_t off = a.spans[2 * k], len = a.spans[2 * k + 1];
      if (off < 41u || off > flen || len > flen - off || flen - off - len < 4u || len > flen - nstream) { st = ST_FRAMING; break; }
      if (be32(file + off - 4) != 0x49444154u) { st = ST_FRAMING; break; }  // "IDAT"
      if (region_crc(s, file, off - 4u, len + 4u, stream + nstream, 4u, lane) != be32(file + off + len)) st = ST_CRC;
      nstream += len;
    }
    st = (int)rfl((uint32_t)st);
    nstream = rfl(nstream);
    if (!st && lane < 4) stream[nstream + lane] = 0;  // the last word's tail
  }
  __syncthreads();

  // ---- 3. inflate
  uint32_t adA = 1, adB = 0;
  if (!st) {
    Bits r;
    r.bb = 0; r.nb = 0; r.iw = 0; r.ibase = 0;
    r.nbytes = nstream;
    r.nwords = (nstream + 3u) >> 2;
    r.words = reinterpret_cast<const uint32_t*>(stream);
    load_input(s, r, lane);
    refill(s, r, lane);
    const uint32_t cmf = take(r, 8), flg = take(r, 8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) st = ST_ZLIB_HEADER;
    uint32_t outpos = 0, flushed = 0;
    bool fixed_ready = false;
    uint32_t last = 0;
    while (!st && !last) {
      refill(s, r, lane);
      last = take(r, 1);
      const uint32_t type = take(r, 2);
      if (exhausted(r)) { st = ST_EXHAUSTED; break; }
      if (type == 3u) { st = ST_BLOCK_TYPE; break; }
      if (type == 0u) {
        take(r, r.nb & 7);
        refill(s, r, lane);
        const uint32_t len = take(r, 16), nlen = take(r, 16);
        if (exhausted(r)) { st = ST_EXHAUSTED; break; }
        if ((len ^ 0xffffu) != nlen) { st = ST_STORED_LEN; break; }
        const uint32_t bp = (uint32_t)(consumed_bits(r) >> 3);
        if (len > nstream - bp) { st = ST_EXHAUSTED; break; }
        if (len > total - outpos) { st = ST_LONG; break; }
        for (uint32_t done = 0; done < len;) {
          const uint32_t m = min(len - done, 4096u);
          for (uint32_t i = lane; i < m; i += 64u) s.ring[(outpos + i) & (CS_PNGDEC_RING - 1)] = stream[bp + done + i];
          outpos += m;
          done += m;
          if (outpos - flushed >= CS_PNGDEC_FLUSH) { flush_ring(s, fil, flushed, CS_PNGDEC_FLUSH, adA, adB, lane); flushed += CS_PNGDEC_FLUSH; }
        }
        seek_byte(s, r, bp + len, lane);
        continue;
      }
      int nl, nd;
      if (type == 1u) {
        nl = 288; nd = 32;
        if (!fixed_ready) {
          __syncthreads();
          for (int i = lane; i < 320; i += 64) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
          build_table(s, s.lens, 288, s.ltab, CS_PNGDEC_PB, s.lcnt, s.lfirst, s.lstart, s.lsyms, false, lane);
          build_table(s, s.lens + 288, 32, s.dtab, CS_PNGDEC_PB, s.dcnt, s.dfirst, s.dstart, s.dsyms, false, lane);
          fixed_ready = true;
        }
      } else {
        fixed_ready = false;
        refill(s, r, lane);
        nl = (int)take(r, 5) + 257;
        nd = (int)take(r, 5) + 1;
        const int nc = (int)take(r, 4) + 4;
        if (nl > 286 || nd > 30) { st = ST_BAD_CODE; break; }
        __syncthreads();
        if (lane < 19) s.lens[lane] = 0;
        __syncthreads();
        for (int i = 0; i < nc; ++i) {
          refill(s, r, lane);
          // the order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
          const unsigned long long ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                                            11ull << 50 | 4ull << 55;
          const unsigned long long ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
          const int pos = i < 12 ? (int)((ord_lo >> (5 * i)) & 31ull) : (int)((ord_hi >> (5 * (i - 12))) & 31ull);
          s.lens[pos] = (uint8_t)take(r, 3);
        }
        if (exhausted(r)) { st = ST_EXHAUSTED; break; }
        st = build_table(s, s.lens, 19, s.dtab, 7, s.dcnt, s.dfirst, s.dstart, s.dsyms, true, lane);
        if (st) break;
        // the nl + nd code lengths, behind the 19 of the code-length code: lens[32 ...)
        uint8_t* cl = s.lens + 32;
        int have = 0, prev = 0;
        while (have < nl + nd) {
          refill(s, r, lane);
          const int sym = decode_sym(r, s.dtab, 7, s.dcnt, s.dfirst, s.dstart, s.dsyms);
          if (sym < 0) { st = ST_BAD_SYMBOL; break; }
          if (sym < 16) { cl[have++] = (uint8_t)sym; prev = sym; continue; }
          int rep, val = 0;
          if (sym == 16) {
            if (have == 0) { st = ST_BAD_CODE; break; }
            val = prev;
            rep = 3 + (int)take(r, 2);
          } else if (sym == 17) {
            rep = 3 + (int)take(r, 3);
          } else {
            rep = 11 + (int)take(r, 7);
          }
          if (have + rep > nl + nd) { st = ST_BAD_CODE; break; }
          for (int k = 0; k < rep; ++k) cl[have + k] = (uint8_t)val;
          have += rep;
          prev = val;
          if (exhausted(r)) { st = ST_EXHAUSTED; break; }
        }
        if (st) break;
        if (exhausted(r)) { st = ST_EXHAUSTED; break; }
        __syncthreads();
        if (rfl(cl[256]) == 0u) { st = ST_BAD_CODE; break; }  // no end-of-block code
        st = build_table(s, cl, nl, s.ltab, CS_PNGDEC_PB, s.lcnt, s.lfirst, s.lstart, s.lsyms, false, lane);
        if (st) break;
        st = build_table(s, cl + nl, nd, s.dtab, CS_PNGDEC_PB, s.dcnt, s.dfirst, s.dstart, s.dsyms, false, lane);
        if (st) break;
      }
      // ---- the symbol loop of one block
      for (;;) {
        refill(s, r, lane);
        if (r.iw > r.nwords + 2u) { st = ST_EXHAUSTED; break; }
        const int sym = decode_sym(r, s.ltab, CS_PNGDEC_PB, s.lcnt, s.lfirst, s.lstart, s.lsyms);
        if (sym < 256) {
          if (sym < 0) { st = ST_BAD_SYMBOL; break; }
          if (outpos >= total) { st = ST_LONG; break; }
          s.ring[outpos & (CS_PNGDEC_RING - 1)] = (uint8_t)sym;
          outpos += 1;
        } else {
          if (sym == 256) break;
          if (sym >= nl || sym >= 286) { st = ST_BAD_SYMBOL; break; }
          uint32_t len;
          if (sym < 265) len = (uint32_t)sym - 254u;
          else if (sym == 285) len = 258u;
          else {
            const int eb = (sym - 261) >> 2;
            len = 3u + ((4u + ((uint32_t)(sym - 261) & 3u)) << eb) + take(r, eb);
          }
          refill(s, r, lane);
          const int dc = decode_sym(r, s.dtab, CS_PNGDEC_PB, s.dcnt, s.dfirst, s.dstart, s.dsyms);
          if (dc < 0 || dc >= nd || dc >= 30) { st = ST_BAD_SYMBOL; break; }
          uint32_t dist;
          if (dc < 4) dist = (uint32_t)dc + 1u;
          else {
            const int eb = (dc >> 1) - 1;
            dist = 1u + ((2u + ((uint32_t)dc & 1u)) << eb) + take(r, eb);
          }
          if (dist > outpos) { st = ST_DISTANCE; break; }
          if (len > total - outpos) { st = ST_LONG; break; }
          // the copy, by all lanes: byte k of the match is byte k mod dist of the dist bytes before it
          __syncthreads();
          const uint32_t src0 = outpos - dist;
          for (uint32_t k0 = 0; k0 < len; k0 += 64u) {
            const uint32_t k = k0 + (uint32_t)lane;
            uint32_t b = 0;
            if (k < len) b = s.ring[(src0 + (dist >= len ? k : k % dist)) & (CS_PNGDEC_RING - 1)];
            if (k < len) s.ring[(outpos + k) & (CS_PNGDEC_RING - 1)] = (uint8_t)b;
          }
          __syncthreads();
          outpos += len;
        }
        if (outpos - flushed >= CS_PNGDEC_FLUSH) { flush_ring(s, fil, flushed, CS_PNGDEC_FLUSH, adA, adB, lane); flushed += CS_PNGDEC_FLUSH; }
      }
      if (!st && exhausted(r)) st = ST_EXHAUSTED;
    }
    if (!st && outpos < total) st = ST_SHORT;
    if (!st) {
      if (outpos > flushed) flush_ring(s, fil, flushed, outpos - flushed, adA, adB, lane);
      take(r, r.nb & 7);
      refill(s, r, lane);
      const uint32_t ad = take(r, 32);
      const uint32_t want = ((ad & 0xffu) << 24) | ((ad & 0xff00u) << 8) | ((ad >> 8) & 0xff00u) | (ad >> 24);
      if (exhausted(r)) st = ST_EXHAUSTED;
      else if (want != ((adB << 16) | adA)) st = ST_ADLER;
    }
  }
  st = (int)rfl((uint32_t)st);
  __syncthreads();

  // ---- 4. un-filter: filter types first, so that a bad one leaves the pixels alone
  if (!st) {
    int bad = 0;
    for (int r = lane; r < a.H; r += 64) bad |= fil[(uint32_t)r * pitch] > 4;
    if (__any(bad)) st = ST_FILTER;
  }
  if (!st) {
    uint32_t* above = reinterpret_cast<uint32_t*>(s.ring);  // the last row of the band before: W <= 4096 pixels of 4 bytes
    uint8_t* dst = a.pixels + (unsigned long long)img * (unsigned long long)a.image_stride;
    const int W = a.W, H = a.H;
    for (int r0 = 0; r0 < H; r0 += 64) {
      const int row = r0 + lane;
      const bool active = row < H;
      const uint8_t* line = fil + (unsigned long long)(active ? row : 0) * pitch;
      const int ft = active ? line[0] : 0;
      uint32_t res = 0, up = 0, ul = 0;
      uint32_t raw_next = 0;
      if (lane == 0 && active)
        for (int j = 0; j < bpp; ++j) raw_next |= (uint32_t)line[1 + j] << (8 * j);
      for (int t = 0; t < W + 63; ++t) {
        const int x = t - lane;
        const bool on = active && x >= 0 && x < W;
        uint32_t from_above = __shfl_up(res, 1, 64);  // lane - 1 was at this x one step ago
        if (lane == 0) from_above = (r0 > 0 && x < W) ? above[x] : 0u;
        ul = up;
        up = from_above;
        const uint32_t raw = raw_next;
        raw_next = 0;
        if (active && x + 1 >= 0 && x + 1 < W)
          for (int j = 0; j < bpp; ++j) raw_next |= (uint32_t)line[1 + (x + 1) * bpp + j] << (8 * j);
        uint32_t out = 0;
        if (on) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t A = (res >> (8 * j)) & 0xffu, B = (up >> (8 * j)) & 0xffu, Cc = (ul >> (8 * j)) & 0xffu, v = (raw >> (8 * j)) & 0xffu;
            const uint32_t pred = ft == 1 ? A : ft == 2 ? B : ft == 3 ? (A + B) >> 1 : ft == 4 ? paeth(A, B, Cc) : 0u;
            out |= ((v + pred) & 0xffu) << (8 * j);
          }
          if (a.kind == 1) {
            uint8_t* p = dst + ((unsigned long long)row * W + x) * 3ull;
            p[0] = (uint8_t)out;
            p[1] = (uint8_t)(bpp == 1 ? out : out >> 8);
            p[2] = (uint8_t)(bpp == 1 ? out : out >> 16);
          } else {
            reinterpret_cast<uint16_t*>(dst)[(unsigned long long)row * W + x] = (uint16_t)(((out & 0xffu) << 8) | ((out >> 8) & 0xffu));
          }
          if (lane == 63) above[x] = out;
        }
        res = out;  // 0 outside the row: the left and upper-left neighbours of pixel 0
      }
      __syncthreads();
    }
  }
  if (lane == 0) a.status[img] = (uint32_t)st;
}

}  // namespace

extern "C" {

// bytes of one file's slot of filtered stream: H * (1 + 4 W) at most, rounded for the 16-byte flushes
static size_t pngdec_fslot(int H, int W) { return (((size_t)H * (1 + 4 * (size_t)W)) + 31) & ~(size_t)15; }

size_t cs_pngdec_workspace(int kind, int I, int H, int W, size_t total_file_bytes) {
  if ((kind != 0 && kind != 1) || I <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)I * pngdec_fslot(H, W) + ((total_file_bytes + 8 * (size_t)I + 16 + 15) & ~(size_t)15);
}

hipError_t cs_pngdec_launch(const uint8_t* files, const unsigned long long* file_offsets, const uint32_t* file_lengths, const uint32_t* spans,
                            const uint32_t* span_offsets, size_t files_bytes, int I, int kind, int H, int W, void* pixels, long long image_stride,
                            uint32_t* status, void* workspace, hipStream_t st) {
  PngDecArgs a;
  a.files = files; a.file_offsets = file_offsets; a.file_lengths = file_lengths; a.spans = spans; a.span_offsets = span_offsets;
  a.files_bytes = files_bytes;
  a.kind = kind; a.H = H; a.W = W;
  a.pixels = (uint8_t*)pixels; a.image_stride = image_stride; a.status = status;
  a.filtered = (uint8_t*)workspace;
  a.fslot = pngdec_fslot(H, W);
  a.streams = (uint8_t*)workspace + (size_t)I * a.fslot;
  hipLaunchKernelGGL(png_decode_kernel, dim3(I), dim3(CS_PNGDEC_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // extern "C"
