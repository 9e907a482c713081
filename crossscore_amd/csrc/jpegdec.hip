// Baseline JPEG decoder on the device (gfx950): compressed files in, uint8 HWC RGB images out.  The sibling of pngdec.hip.
//
// Three launches per call, whatever the number of files:
//   1. entropy   one workgroup of four waves per file.  Thread 0 walks the header once (SOF0, DQT, DHT, DRI, SOS; everything the host's probe
//                said is read again here) and leaves the quantisation tables and the canonical Huffman tables in LDS, validated while they are
//                built; all threads fill the 9-bit primary lookups.  With a restart interval, a ballot / popcount pass over the scan bytes builds
//                the ordered table of RSTn positions in the workspace, and their count and numbering are checked before anything is decoded.
//                Wave w then decodes restart intervals w, w + 4, ...: each starts at a known byte and a known MCU with zero predictors.  The
//                symbol loop's state (bit buffer, positions, predictors) is wave-uniform; the scan is staged through a 256-byte window per wave
//                in LDS; a block is assembled in LDS and leaves as one coalesced store of 64 dequantised int16 (natural order, saturated) into
//                the component's block-major coefficient plane.  Without DRI wave 0 decodes the file alone.
//   2. IDCT      jpeg_idct_islow in integers (CONST_BITS 13, PASS1_BITS 2): eight threads per block, columns, a transpose through LDS, rows;
//                uint8 sample planes padded to whole blocks.
//   3. pixels    one thread per pixel: "fancy" (triangle) chroma upsampling of 4:2:2 / 4:2:0 from the REAL chroma rows and columns, the 16-bit
//                fixed-point YCbCr -> RGB conversion, stores for y < H, x < W only.
// Stages 2 and 3 do nothing for a file whose status word is not zero, so such a file writes no pixel.
//
// Untrusted input: every read of a file is at an index below its length; the bit reader hands out zeros past the end of an interval and the
// loops stop on "input exhausted"; the MCU and block counts come from the call's H, W and the sampling (1 or 2), never from a length in the
// file, so coefficient stores stay inside the file's own planes; the restart table holds at most MCUs - 1 entries, which its slot has.
#include "jpeg_shared.h"

namespace {

struct JpgLds {
  uint16_t look[4][1 << CS_JPGDEC_PB];  // per table (DC0, DC1, AC0, AC1): symbol | length << 8, 0 = walk the canonical code
  uint32_t first[4][17];                // per code length: first code
  uint16_t cnt[4][17], start[4][17];    // ... number of codes, index of its first symbol
  uint16_t nsym[4];
  uint8_t syms[4][256];
  uint8_t qt[4][64];  // zig-zag order, as the file has them
  uint8_t zz[64];
  int16_t blk[4][64];   // one block per wave
  uint32_t inw[4][64];  // one 256-byte window of the scan per wave
  uint32_t wcnt[2][4], wterm[2][4];
  uint32_t hdr[16];
  int status;
};

__device__ __forceinline__ Huff huff_of(JpgLds& s, int t) { return Huff{s.look[t], s.first[t], s.cnt[t], s.start[t], s.syms[t]}; }

enum { ST_OTHER_PROCESS = -1 };  // parse_header: a SOF2 file in a call that has the progressive kernel behind this one

enum { HD_NCOMP = 0, HD_HS, HD_VS, HD_RI, HD_SCAN, HD_TQ, HD_TD, HD_TA };  // HD_TQ / TD / TA: one byte per component

// The header, by one thread: 0 or a status.  Reads below flen only.
__device__ int parse_header(JpgLds& s, const uint8_t* file, uint32_t flen, int H, int W, int flags) {
  if (flen < 4u || file[0] != 0xFF || file[1] != 0xD8) return ST_FRAMING;
  uint32_t pos = 2, ri = 0, qdef = 0, hdef = 0;
  int nc = 0, hs = 1, vs = 1;
  bool have_sof = false, jfif = false;
  uint32_t id[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
  for (;;) {
    if (flen - pos < 4u) return ST_FRAMING;  // no SOS
    if (file[pos] != 0xFF) return ST_FRAMING;
    const uint32_t m = file[pos + 1];
    if (m == 0xFF) { pos += 1; continue; }  // a fill byte
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return ST_FRAMING;
    const uint32_t len = be16(file + pos + 2);
    if (len < 2u || len > flen - pos - 2u) return ST_FRAMING;
    const uint32_t seg = pos + 4, send = pos + 2 + len;
    if (m == 0xC0) {
      if (have_sof || len < 8u) return ST_FRAMING;
      nc = file[seg + 5];
      if (len != 8u + 3u * (uint32_t)nc) return ST_FRAMING;
      if (file[seg] != 8 || (nc != 1 && nc != 3)) return ST_HEADER;
      if (be16(file + seg + 1) != (uint32_t)H || be16(file + seg + 3) != (uint32_t)W) return ST_HEADER;
      for (int c = 0; c < nc; ++c) {
        id[c] = file[seg + 6 + 3 * c];
        const uint32_t hv = file[seg + 7 + 3 * c];
        tq[c] = file[seg + 8 + 3 * c];
        if (tq[c] > 3u) return ST_TABLE;
        if (c == 0) {
          if (hv != 0x11 && (nc == 1 || (hv != 0x21 && hv != 0x22))) return ST_HEADER;
          hs = (int)(hv >> 4); vs = (int)(hv & 15u);
        } else if (hv != 0x11) {
          return ST_HEADER;
        }
      }
      if (hs == 2 && W <= 4) return ST_HEADER;  // libjpeg's replication upsampler: not built
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      if (m == 0xC2 && (flags & CS_JPGDEC_PROGRESSIVE)) return ST_OTHER_PROCESS;
      return ST_HEADER;  // another process (progressive, extended, lossless, arithmetic)
    } else if (m == 0xC4) {
      uint32_t p = seg;
      while (p < send) {
        if (send - p < 17u) return ST_TABLE;
        const uint32_t tc = file[p] >> 4, th = file[p] & 15u;
        if (tc > 1u || th > 1u) return ST_TABLE;
        const int t = (int)(tc * 2u + th);
        uint32_t total = 0;
        if (huff_define(huff_of(s, t), file, p, send, &total)) return ST_TABLE;
        s.nsym[t] = (uint16_t)total;
        hdef |= 1u << t;
        p += 17u + total;
      }
    } else if (m == 0xDB) {
      uint32_t p = seg;
      while (p < send) {
        if (send - p < 65u) return ST_TABLE;
        const uint32_t pq = file[p] >> 4, t = file[p] & 15u;
        if (pq != 0u || t > 3u) return ST_TABLE;
        for (int j = 0; j < 64; ++j) s.qt[t][j] = file[p + 1 + j];
        qdef |= 1u << t;
        p += 65u;
      }
    } else if (m == 0xDD) {
      if (len != 4u) return ST_FRAMING;
      ri = be16(file + seg);
    } else if (m == 0xE0) {
      if (len >= 7u && file[seg] == 'J' && file[seg + 1] == 'F' && file[seg + 2] == 'I' && file[seg + 3] == 'F' && file[seg + 4] == 0) jfif = true;
    } else if (m == 0xEE) {
      if (len >= 7u && file[seg] == 'A' && file[seg + 1] == 'd' && file[seg + 2] == 'o' && file[seg + 3] == 'b' && file[seg + 4] == 'e') return ST_HEADER;
    } else if (m == 0xDA) {
      if (!have_sof || len < 3u) return ST_FRAMING;
      const int ns = file[seg];
      if (len != 6u + 2u * (uint32_t)ns) return ST_FRAMING;
      if (ns != nc) return ST_HEADER;
      if (nc == 3 && !jfif && !(id[0] == 1u && id[1] == 2u && id[2] == 3u)) return ST_HEADER;
      uint32_t ptq = 0, ptd = 0, pta = 0;
      for (int c = 0; c < nc; ++c) {
        if (file[seg + 1 + 2 * c] != id[c]) return ST_HEADER;
        const uint32_t td = file[seg + 2 + 2 * c] >> 4, ta = file[seg + 2 + 2 * c] & 15u;
        if (td > 1u || ta > 1u) return ST_TABLE;
        if (!((hdef >> td) & 1u) || !((hdef >> (2u + ta)) & 1u) || !((qdef >> tq[c]) & 1u)) return ST_TABLE;  // selected, never defined
        ptq |= tq[c] << (8 * c); ptd |= td << (8 * c); pta |= (2u + ta) << (8 * c);
      }
      if (file[seg + 1 + 2 * nc] != 0 || file[seg + 2 + 2 * nc] != 63 || file[seg + 3 + 2 * nc] != 0) return ST_HEADER;
      s.hdr[HD_NCOMP] = (uint32_t)nc; s.hdr[HD_HS] = (uint32_t)hs; s.hdr[HD_VS] = (uint32_t)vs; s.hdr[HD_RI] = ri; s.hdr[HD_SCAN] = send;
      s.hdr[HD_TQ] = ptq; s.hdr[HD_TD] = ptd; s.hdr[HD_TA] = pta;
      return ST_OK;
    }
    pos = send;
  }
}

__global__ __launch_bounds__(CS_JPGDEC_THREADS) void jpeg_entropy_kernel(CsJpgDecArgs a) {
  __shared__ __attribute__((aligned(16))) JpgLds s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = (int)rfl((uint32_t)(tid >> 6));
  const int img = blockIdx.x;

  const unsigned long long foff = a.file_offsets[img];
  const uint32_t flen = a.file_lengths[img];
  const bool framed = flen >= 4u && flen < (1u << 28) && foff <= a.files_bytes && (unsigned long long)flen <= a.files_bytes - foff;
  const uint8_t* file = a.files + (framed ? foff : 0ull);

  zigzag_to_lds(s.zz, tid);
  for (int k = tid; k < 4 * (1 << CS_JPGDEC_PB); k += CS_JPGDEC_THREADS) (&s.look[0][0])[k] = 0;
  if (tid < 4) s.nsym[tid] = 0;
  if (tid == 0) s.status = ST_OK;
  __syncthreads();

  // ---- the header: tables into LDS
  if (tid == 0) s.status = framed ? parse_header(s, file, flen, a.H, a.W, a.flags) : ST_FRAMING;
  __syncthreads();
  if (s.status != ST_OK) {  // uniform over the workgroup
    if (tid == 0) a.status[img] = s.status == ST_OTHER_PROCESS ? CS_JPGDEC_PENDING : (uint32_t)s.status;  // pending: jpegprog.hip's file
    return;
  }
  for (int t = 0; t < 4; ++t) huff_fill_lookup(huff_of(s, t), s.nsym[t], tid, CS_JPGDEC_THREADS);
  __syncthreads();

  const Geometry g = geometry(a.H, a.W, (int)s.hdr[HD_NCOMP], (int)s.hdr[HD_HS], (int)s.hdr[HD_VS]);
  const uint32_t total = (uint32_t)g.mcux * (uint32_t)g.mcuy;  // bounded by the call's H, W: <= 512 * 512
  const uint32_t ri = s.hdr[HD_RI] ? min(s.hdr[HD_RI], total) : total;
  const uint32_t nint = (total + ri - 1u) / ri;
  const uint32_t scan = s.hdr[HD_SCAN];
  uint32_t* rst = a.rst + (unsigned long long)img * a.rst_slot;  // nint - 1 <= total - 1 < rst_slot entries
  uint32_t scan_end = flen;

  // ---- the restart markers, in file order: count and numbering before anything is decoded
  if (nint > 1u) {
    uint32_t count = 0;
    int misnumbered = 0;
    restart_positions(file, flen, scan, nint, rst, s.wcnt, s.wterm, tid, lane, wave, scan_end, count, misnumbered);
    if (misnumbered || count != nint - 1u) atomicCAS(&s.status, ST_OK, ST_RESTART);
    __syncthreads();
    if (s.status != ST_OK) {
      if (tid == 0) a.status[img] = (uint32_t)s.status;
      return;
    }
  }

  // ---- the symbol loop: wave w takes intervals w, w + 4, ...
  {
    Bits r;
    r.file = file; r.flen = flen; r.win = s.inw[wave];
    int16_t* blk = s.blk[wave];
    int16_t* coef = a.coef + (unsigned long long)img * a.blocks_slot * 64ull;
    const uint32_t ptq = s.hdr[HD_TQ], ptd = s.hdr[HD_TD], pta = s.hdr[HD_TA];
    int st = ST_OK;
    for (uint32_t k = (uint32_t)wave; k < nint && !st; k += 4u) {
      if (rfl((uint32_t)*(volatile int*)&s.status) != 0u) break;  // another wave has ended the file
      const uint32_t start = k == 0u ? scan : rfl(rst[k - 1u]) + 2u;
      const uint32_t end = k + 1u < nint ? rfl(rst[k]) : scan_end;
      start_interval(r, min(start, flen), min(end, flen), lane);
      int pred[3] = {0, 0, 0};
      const uint32_t m1 = min(total, (k + 1u) * ri);
      for (uint32_t m = k * ri; m < m1 && !st; ++m) {
        const int my = (int)(m / (uint32_t)g.mcux), mx = (int)(m % (uint32_t)g.mcux);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c >= g.ncomp || st) continue;
          const int hc = c == 0 ? g.hs : 1, vc = c == 0 ? g.vs : 1;
          const int tq = (int)((ptq >> (8 * c)) & 255u), td = (int)((ptd >> (8 * c)) & 255u), ta = (int)((pta >> (8 * c)) & 255u);
          for (int b = 0; b < hc * vc && !st; ++b) {
            const int by = my * vc + b / hc, bx = mx * hc + b % hc;  // by < bh[c], bx < bw[c]
            blk[lane] = 0;
            wave_sync();
            refill(r, lane);
            int sym = decode_sym(huff_of(s, td), r);
            if (sym < 0) st = ST_CODE;
            else if (sym > 11) st = ST_SYMBOL;
            else if (sym) pred[c] += extend(take(r, sym), sym);
            if (lane == 0) blk[0] = (int16_t)sat16(pred[c] * (int)s.qt[tq][0]);
            int kk = 1;
            while (kk < 64 && !st) {
              refill(r, lane);
              sym = decode_sym(huff_of(s, ta), r);
              if (sym < 0) { st = ST_CODE; break; }
              const int run = sym >> 4, size = sym & 15;
              if (size == 0) {
                if (run != 15) break;  // EOB
                kk += 16;
                continue;
              }
              kk += run;
              if (kk > 63 || size > 10) { st = ST_SYMBOL; break; }
              const int v = extend(take(r, size), size);
              if (lane == 0) blk[rfl(s.zz[kk])] = (int16_t)sat16(v * (int)rfl(s.qt[tq][kk]));
              kk += 1;
            }
            if (r.nb < r.fake || (st && r.nb - 16 < r.fake)) st = ST_EXHAUSTED;  // an error read from the zeros behind the data is the data's end
            if (st) break;
            wave_sync();
            coef[((unsigned long long)g.off[c] + (unsigned long long)by * (unsigned)g.bw[c] + (unsigned)bx) * 64ull + (unsigned)lane] = blk[lane];
          }
        }
      }
    }
    if (st && lane == 0) atomicCAS(&s.status, ST_OK, st);
  }
  __syncthreads();
  if (tid == 0) {
    a.status[img] = (uint32_t)s.status;
    uint32_t* info = a.info + 4ull * (unsigned)img;
    info[0] = (uint32_t)g.ncomp; info[1] = (uint32_t)g.hs; info[2] = (uint32_t)g.vs; info[3] = 0u;
  }
}

// ---- jpeg_idct_islow
constexpr uint32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137,
                   F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// eight inputs -> eight outputs, before the descale; unsigned arithmetic, so that wrap-around is defined
__device__ __forceinline__ void idct8(const uint32_t c[8], uint32_t o[8]) {
  uint32_t z1 = (c[2] + c[6]) * F_0_541;
  const uint32_t e2 = z1 - c[6] * F_1_847, e3 = z1 + c[2] * F_0_765;
  const uint32_t e0 = (c[0] + c[4]) << 13, e1 = (c[0] - c[4]) << 13;
  const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  uint32_t t0 = c[7], t1 = c[5], t2 = c[3], t3 = c[1];
  z1 = t0 + t3;
  uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * F_1_175;
  t0 *= F_0_298; t1 *= F_2_053; t2 *= F_3_072; t3 *= F_1_501;
  z1 *= 0u - F_0_899; z2 *= 0u - F_2_562;
  z3 = z3 * (0u - F_1_961) + z5;
  z4 = z4 * (0u - F_0_390) + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  o[0] = t10 + t3; o[7] = t10 - t3;
  o[1] = t11 + t2; o[6] = t11 - t2;
  o[2] = t12 + t1; o[5] = t12 - t1;
  o[3] = t13 + t0; o[4] = t13 - t0;
}

__device__ __forceinline__ uint32_t descale(uint32_t x, int n) { return (uint32_t)((int32_t)(x + (1u << (n - 1))) >> n); }

__global__ __launch_bounds__(CS_JPGDEC_THREADS) void jpeg_idct_kernel(CsJpgDecArgs a) {
  __shared__ uint32_t ws[32][65];  // 32 blocks between the passes, padded against bank conflicts
  const int img = blockIdx.y;
  if (a.status[img] != 0u) return;  // uniform over the workgroup
  const uint32_t* info = a.info + 4ull * (unsigned)img;
  const Geometry g = geometry(a.H, a.W, (int)info[0], (int)info[1], (int)info[2]);
  const int tid = threadIdx.x, q = tid >> 3, j = tid & 7;
  const uint32_t b = blockIdx.x * 32u + (uint32_t)q;
  const bool on = b < g.nblocks;
  const int16_t* coef = a.coef + ((unsigned long long)img * a.blocks_slot + (on ? b : 0u)) * 64ull;
  uint32_t c[8], o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) c[r] = on ? (uint32_t)(int32_t)coef[r * 8 + j] : 0u;  // column j
  idct8(c, o);
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[q][r * 8 + j] = descale(o[r], 11);
  __syncthreads();
  if (!on) return;
#pragma unroll
  for (int r = 0; r < 8; ++r) c[r] = ws[q][j * 8 + r];  // row j
  idct8(c, o);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int v = (int32_t)descale(o[r], 18) + 128;
    const uint32_t u = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    if (r < 4) lo |= u << (8 * r); else hi |= u << (8 * (r - 4));
  }
  const int comp = b < g.off[1] ? 0 : b < g.off[2] ? 1 : 2;
  const uint32_t lb = b - g.off[comp];
  const uint32_t by = lb / (uint32_t)g.bw[comp], bx = lb % (uint32_t)g.bw[comp];
  // plane `comp` starts at sample off[comp] * 64, rows of bw * 8 samples: 8-byte aligned stores
  uint8_t* dst = a.samples + (unsigned long long)img * a.blocks_slot * 64ull + (unsigned long long)g.off[comp] * 64ull +
                 ((unsigned long long)by * 8ull + (unsigned)j) * ((unsigned long long)g.bw[comp] * 8ull) + (unsigned long long)bx * 8ull;
  *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// ---- upsampling and colour
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// chroma sample for pixel (y, x) of a plane with `rows` x `n` real samples, `pitch` bytes a row
__device__ __forceinline__ int chroma_at(const uint8_t* p, int pitch, int rows, int n, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(long long)y * pitch + x];
  const int j = x >> 1;
  if (vs == 1) {
    const uint8_t* in = p + (long long)y * pitch;
    if (x == 0) return in[0];
    if (x == 2 * n - 1) return in[n - 1];
    return (x & 1) ? (3 * in[j] + in[j + 1] + 2) >> 2 : (3 * in[j] + in[j - 1] + 1) >> 2;
  }
  const int i = y >> 1;
  const int o = (y & 1) ? min(i + 1, rows - 1) : max(i - 1, 0);
  const uint8_t* in = p + (long long)i * pitch;
  const uint8_t* ot = p + (long long)o * pitch;
  const int sj = 3 * in[j] + ot[j];
  if (x == 0) return (4 * sj + 8) >> 4;
  if (x == 2 * n - 1) return (4 * sj + 7) >> 4;
  if (x & 1) return (3 * sj + (3 * in[j + 1] + ot[j + 1]) + 7) >> 4;
  return (3 * sj + (3 * in[j - 1] + ot[j - 1]) + 8) >> 4;
}

__global__ __launch_bounds__(CS_JPGDEC_THREADS) void jpeg_pixels_kernel(CsJpgDecArgs a) {
  const int img = blockIdx.y;
  if (a.status[img] != 0u) return;
  const unsigned long long idx = (unsigned long long)blockIdx.x * CS_JPGDEC_THREADS + threadIdx.x;
  if (idx >= (unsigned long long)a.H * (unsigned)a.W) return;
  const int y = (int)(idx / (unsigned)a.W), x = (int)(idx % (unsigned)a.W);
  const uint32_t* info = a.info + 4ull * (unsigned)img;
  const Geometry g = geometry(a.H, a.W, (int)info[0], (int)info[1], (int)info[2]);
  const uint8_t* base = a.samples + (unsigned long long)img * a.blocks_slot * 64ull;
  const int Y = base[(long long)y * (g.bw[0] * 8) + x];
  int R = Y, G = Y, B = Y;
  if (g.ncomp == 3) {
    const int rows = (a.H + g.vs - 1) / g.vs, n = (a.W + g.hs - 1) / g.hs, pitch = g.bw[1] * 8;
    const int cb = chroma_at(base + (unsigned long long)g.off[1] * 64ull, pitch, rows, n, g.hs, g.vs, y, x) - 128;
    const int cr = chroma_at(base + (unsigned long long)g.off[2] * 64ull, pitch, rows, n, g.hs, g.vs, y, x) - 128;
    R = clamp255(Y + ((91881 * cr + 32768) >> 16));
    G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    B = clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
  uint8_t* p = a.pixels + (unsigned long long)img * (unsigned long long)a.image_stride + idx * 3ull;
  p[0] = (uint8_t)R;
  p[1] = (uint8_t)G;
  p[2] = (uint8_t)B;
}

}  // namespace

extern "C" {

// blocks of one file's slot: three planes padded to 16 x 16 pixels hold every accepted sampling
static size_t jpgdec_blocks(int H, int W) { return 12 * (size_t)((H + 15) / 16) * (size_t)((W + 15) / 16); }
static size_t jpgdec_rst_slot(int H, int W) { return (((size_t)((H + 7) / 8) * (size_t)((W + 7) / 8)) + 3) & ~(size_t)3; }
static size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// flags & CS_JPGDEC_PROGRESSIVE: behind everything else, one restart table per scan of each file (its size from H, W, I alone)
size_t cs_jpgdec_workspace(int I, int H, int W, int flags) {
  if (I <= 0 || H <= 0 || W <= 0) return 0;
  const size_t base = round16((size_t)I * 16) + (size_t)I * jpgdec_rst_slot(H, W) * 4 + (size_t)I * jpgdec_blocks(H, W) * (128 + 64);
  return base + ((flags & CS_JPGDEC_PROGRESSIVE) ? (size_t)I * CS_JPGDEC_MAX_SCANS * jpgdec_rst_slot(H, W) * 4 : 0);
}

hipError_t cs_jpgdec_launch(const uint8_t* files, const unsigned long long* file_offsets, const uint32_t* file_lengths, size_t files_bytes, int I,
                            int H, int W, void* pixels, long long image_stride, uint32_t* status, void* workspace, int flags, int levels,
                            hipStream_t st) {
  CsJpgDecArgs a;
  a.files = files; a.file_offsets = file_offsets; a.file_lengths = file_lengths; a.files_bytes = files_bytes;
  a.H = H; a.W = W;
  a.pixels = (uint8_t*)pixels; a.image_stride = image_stride; a.status = status;
  uint8_t* w = (uint8_t*)workspace;
  a.info = (uint32_t*)w;
  w += round16((size_t)I * 16);
  a.rst = (uint32_t*)w;
  a.rst_slot = jpgdec_rst_slot(H, W);
  w += (size_t)I * a.rst_slot * 4;
  a.blocks_slot = jpgdec_blocks(H, W);
  a.coef = (int16_t*)w;
  w += (size_t)I * a.blocks_slot * 128;
  a.samples = w;
  w += (size_t)I * a.blocks_slot * 64;
  a.flags = flags; a.levels = levels;
  a.scan_rst = (flags & CS_JPGDEC_PROGRESSIVE) ? (uint32_t*)w : nullptr;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(I), dim3(CS_JPGDEC_THREADS), 0, st, a);
  if (flags & CS_JPGDEC_PROGRESSIVE) {  // each file goes to the entropy kernel of its own process
    const hipError_t e = cs_jpgprog_launch(a, I, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((a.blocks_slot + 31) / 32), I), dim3(CS_JPGDEC_THREADS), 0, st, a);
  hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)(((size_t)H * W + CS_JPGDEC_THREADS - 1) / CS_JPGDEC_THREADS), I), dim3(CS_JPGDEC_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // extern "C"
