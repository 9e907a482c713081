// Progressive JPEG entropy decoder on the device (gfx950): the second entropy launch of cs_op_jpeg_decode_ex with CS_JPEG_PROGRESSIVE.  It
// leaves what jpegdec.hip's entropy stage leaves -- dequantised int16 coefficients in natural order in the file's planes, the info words, the
// status word -- so the IDCT and pixel launches behind it run unchanged.  The baseline entropy kernel marks a SOF2 file "pending" in its
// status word; this kernel takes exactly those files and leaves every other one at once.
//
// One workgroup of four waves per file.
//   scan table   Thread 0 walks every segment of the file (SOF2, DQT, DHT, DRI, SOS ... EOI; nothing the host's probe said is trusted) and
//                fills an LDS table of at most 32 scans: components, Ss, Se, Ah, Al, table selectors, the file offsets of the DHT definitions
//                in force, the unit count and the restart interval.  Behind each SOS all 256 threads run the ballot pass over the scan's
//                bytes: it finds the scan's end (where thread 0 goes on) and its RSTn positions, whose count and numbering are checked.  Each
//                scan is checked against T.81 G.1.1.1.1 and at EOI the progression has to be complete: CS_JPGDEC_BAD_SCAN otherwise.
//   levels       Scan k depends on the earlier scans that touch one of its components and overlap its band (an AC scan also on the component's
//                first DC scan); level = 1 + max(level of those).
//                Levels run in order with a workgroup barrier between them.  Inside a level the items -- a scan, or a (scan, restart interval)
//                pair -- are dealt round-robin to the waves.  No wave waits on another except at those barriers; every wave reaches every
//                barrier whatever status has been set (waves skip work after an error, not barriers); there is no spinning on flags.
//   symbol loop  Wave-uniform state as in the baseline kernel (64-bit bit buffer, 256-byte window in LDS).  Each wave has its own LDS slice for
//                the two Huffman tables of its current scan, built when the scan is decoded, because files redefine tables between scans.
//                Coefficients accumulate as raw int16 in zig-zag order in the file's planes, zeroed before the first level:
//                  DC first        (pred + diff) << Al
//                  DC refinement   one raw bit per block, OR-ed in at 1 << Al
//                  AC first        run/size symbols into the band at << Al; EOBRUN = (1 << r) + bits(r) - 1; a run skips its blocks at once
//                  AC refinement   T.81 G.1.2.3: lane k holds coefficient k of the block, a ballot gives the non-zero history as one 64-bit
//                                  mask, the scalar loop over the band collects correction bits and new +-1 positions as masks, and one vector
//                                  step applies them before the block is stored back.  The next block's load is in flight meanwhile.
//                A non-interleaved scan runs over the component's own ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order (MCU padding blocks
//                are not visited and stay zero), an interleaved DC scan in MCU order; a restart interval counts those units and resets the
//                predictors and the end-of-band run.
//   finish       Each coefficient times its quantiser, saturated to int16, to its natural position.
//
// Untrusted input: reads of the file stay below its length; block indices come from the call's H, W and the frame's sampling; an end-of-band
// run is clipped to the blocks left in its interval; every loop is bounded by the band, the scan's blocks or its bytes; a block that consumed
// bits past the scan's end is "input exhausted"; scan k's restart table has (units of a scan) - 1 < rst_slot entries at most, in its own slot.
#include "jpeg_shared.h"

namespace {

struct ScanEnt {
  uint32_t start, end;          // the scan's entropy-coded bytes
  uint32_t tab[2], tab_end[2];  // per table id: the DHT definition in force (offset of its Tc / Th byte, end of its segment)
  uint32_t units, ri, nint;     // blocks or MCUs of the scan, units per interval, intervals
  uint8_t ns, comp[3], sel[3], ss, se, ah, al, level;
};

struct ProgLds {
  uint16_t look[4][2][1 << CS_JPGDEC_PB];  // per wave: the two tables of its current scan
  uint32_t first[4][2][17];
  uint16_t cnt[4][2][17], start[4][2][17];
  uint8_t syms[4][2][256];
  uint32_t inw[4][64];  // one 256-byte window of the scan per wave
  uint8_t qt[4][64];    // zig-zag order, as the file has them
  uint8_t zz[64];
  ScanEnt scan[CS_JPGDEC_MAX_SCANS];
  uint32_t wcnt[2][4], wterm[2][4];
  // thread 0's walk
  int8_t coded[3][64];  // per coefficient the Al it was last coded with, -1 before its first scan
  uint32_t pos, ri, qdef, dht[4], dht_end[4], id[3], tq[3];
  int nc, hs, vs, have_sof, jfif, nscans, nlevels, done;
  int status;
};

__device__ __forceinline__ Huff huff_of(ProgLds& s, int wave, int t) {
  return Huff{s.look[wave][t], s.first[wave][t], s.cnt[wave][t], s.start[wave][t], s.syms[wave][t]};
}

// blocks across and down of component c's own raster (no MCU padding)
__device__ __forceinline__ void own_blocks(int H, int W, int c, int hs, int vs, int& bwc, int& bhc) {
  const int wc = c == 0 ? W : (W + hs - 1) / hs, hc = c == 0 ? H : (H + vs - 1) / vs;
  bwc = (wc + 7) / 8;
  bhc = (hc + 7) / 8;
}

// block `unit` of a component's own raster of bwc blocks across, in a plane of `pitch` blocks across
__device__ __forceinline__ int16_t* own_block(int16_t* plane, uint32_t unit, uint32_t bwc, uint32_t pitch) {
  return plane + ((unsigned long long)(unit / bwc) * pitch + (unit % bwc)) * 64ull;
}

// a plane's pitch in blocks and its first block, without indexing the arrays by a run-time component (that would put them in scratch)
__device__ __forceinline__ uint32_t pitch_of(const Geometry& g, int c) { return (uint32_t)(c == 0 ? g.bw[0] : g.bw[1]); }
__device__ __forceinline__ uint32_t first_of(const Geometry& g, int c) { return c == 0 ? 0u : c == 1 ? g.off[1] : g.off[2]; }

// Thread 0: from s.pos on to the next SOS (one more entry of s.scan, s.pos at its data) or to EOI (s.done; levels assigned).  0 or a status.
__device__ int walk(ProgLds& s, const uint8_t* file, uint32_t flen, int H, int W, int levels) {
  uint32_t pos = s.pos;
  for (;;) {
    if (s.nscans > 0 && flen - pos >= 2u && file[pos] == 0xFF && file[pos + 1] == 0xD9) {  // EOI
      for (int c = 0; c < s.nc; ++c)
        for (int k = 0; k < 64; ++k)
          if (s.coded[c][k] != 0) return ST_SCAN;  // an incomplete progression
      int top = 0;
      for (int k = 0; k < s.nscans; ++k) {
        int lv = 1;
        for (int j = 0; j < k && levels; ++j) {
          bool shares = false;
          for (int a = 0; a < s.scan[k].ns; ++a)
            for (int b = 0; b < s.scan[j].ns; ++b) shares |= s.scan[k].comp[a] == s.scan[j].comp[b];
          const bool overlap = s.scan[k].ss <= s.scan[j].se && s.scan[j].ss <= s.scan[k].se;
          const bool first_dc = s.scan[k].ss > 0 && s.scan[j].ss == 0 && s.scan[j].ah == 0;  // G.1.1.1.1 orders AC behind the component's first DC scan
          if (shares && (overlap || first_dc)) lv = max(lv, (int)s.scan[j].level + 1);
        }
        if (!levels) lv = k + 1;
        s.scan[k].level = (uint8_t)lv;
        top = max(top, lv);
      }
      s.nlevels = top;
      s.done = 1;
      return ST_OK;
    }
    if (flen - pos < 4u) return ST_FRAMING;  // no SOS, or no EOI
    if (file[pos] != 0xFF) return ST_FRAMING;
    const uint32_t m = file[pos + 1];
    if (m == 0xFF) { pos += 1; continue; }  // a fill byte
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return ST_FRAMING;
    const uint32_t len = be16(file + pos + 2);
    if (len < 2u || len > flen - pos - 2u) return ST_FRAMING;
    const uint32_t seg = pos + 4, send = pos + 2 + len;
    if (m == 0xC2) {
      if (s.have_sof || len < 8u) return ST_FRAMING;
      const int nc = file[seg + 5];
      if (len != 8u + 3u * (uint32_t)nc) return ST_FRAMING;
      if (file[seg] != 8 || (nc != 1 && nc != 3)) return ST_HEADER;
      if (be16(file + seg + 1) != (uint32_t)H || be16(file + seg + 3) != (uint32_t)W) return ST_HEADER;
      int hs = 1, vs = 1;
      for (int c = 0; c < nc; ++c) {
        s.id[c] = file[seg + 6 + 3 * c];
        const uint32_t hv = file[seg + 7 + 3 * c];
        s.tq[c] = file[seg + 8 + 3 * c];
        if (s.tq[c] > 3u) return ST_TABLE;
        if (c == 0) {
          if (hv != 0x11 && (nc == 1 || (hv != 0x21 && hv != 0x22))) return ST_HEADER;
          hs = (int)(hv >> 4); vs = (int)(hv & 15u);
        } else if (hv != 0x11) {
          return ST_HEADER;
        }
      }
      if (hs == 2 && W <= 4) return ST_HEADER;  // libjpeg's replication upsampler: not built
      s.nc = nc; s.hs = hs; s.vs = vs;
      s.have_sof = 1;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      return s.have_sof ? ST_FRAMING : ST_HEADER;  // a second frame header, or another process
    } else if (m == 0xC4) {
      uint32_t p = seg;
      while (p < send) {  // the definitions are only located here: a scan that selects one builds and checks it
        if (send - p < 17u) return ST_TABLE;
        const uint32_t tc = file[p] >> 4, th = file[p] & 15u;
        if (tc > 1u || th > 1u) return ST_TABLE;
        uint32_t total = 0;
        for (int l = 1; l <= 16; ++l) total += file[p + l];
        if (total > 256u || 17u + total > send - p) return ST_TABLE;
        s.dht[tc * 2u + th] = p;
        s.dht_end[tc * 2u + th] = send;
        p += 17u + total;
      }
    } else if (m == 0xDB) {
      if (s.nscans > 0) return ST_SCAN;  // libjpeg latches the tables per component: not behind the first SOS
      uint32_t p = seg;
      while (p < send) {
        if (send - p < 65u) return ST_TABLE;
        const uint32_t pq = file[p] >> 4, t = file[p] & 15u;
        if (pq != 0u || t > 3u) return ST_TABLE;
        for (int j = 0; j < 64; ++j) s.qt[t][j] = file[p + 1 + j];
        s.qdef |= 1u << t;
        p += 65u;
      }
    } else if (m == 0xDD) {
      if (s.nscans > 0) return ST_SCAN;
      if (len != 4u) return ST_FRAMING;
      s.ri = be16(file + seg);
    } else if (m == 0xE0) {
      if (len >= 7u && file[seg] == 'J' && file[seg + 1] == 'F' && file[seg + 2] == 'I' && file[seg + 3] == 'F' && file[seg + 4] == 0) s.jfif = 1;
    } else if (m == 0xEE) {
      if (len >= 7u && file[seg] == 'A' && file[seg + 1] == 'd' && file[seg + 2] == 'o' && file[seg + 3] == 'b' && file[seg + 4] == 'e') return ST_HEADER;
    } else if (m == 0xDA) {
      if (!s.have_sof || len < 3u) return ST_FRAMING;
      const int ns = file[seg];
      if (len != 6u + 2u * (uint32_t)ns) return ST_FRAMING;
      if (s.nc == 3 && !s.jfif && !(s.id[0] == 1u && s.id[1] == 2u && s.id[2] == 3u)) return ST_HEADER;
      if (s.nscans == CS_JPGDEC_MAX_SCANS || ns < 1 || ns > s.nc) return ST_SCAN;
      ScanEnt& e = s.scan[s.nscans];
      e.tab[0] = e.tab[1] = e.tab_end[0] = e.tab_end[1] = 0u;
      const uint32_t ss = file[seg + 1 + 2 * ns], se = file[seg + 2 + 2 * ns], ah = file[seg + 3 + 2 * ns] >> 4, al = file[seg + 3 + 2 * ns] & 15u;
      if (ss == 0u ? se != 0u : (ns != 1 || ss > se || se > 63u)) return ST_SCAN;
      if (al > 13u || (ah != 0u && ah != al + 1u)) return ST_SCAN;
      int prev = -1;
      for (int i = 0; i < ns; ++i) {
        int c = prev + 1;
        while (c < s.nc && s.id[c] != file[seg + 1 + 2 * i]) ++c;
        if (c >= s.nc) return ST_SCAN;  // not a subset of the frame's components, in order
        const uint32_t td = file[seg + 2 + 2 * i] >> 4, ta = file[seg + 2 + 2 * i] & 15u;
        if (td > 1u || ta > 1u) return ST_TABLE;
        if (!((s.qdef >> s.tq[c]) & 1u)) return ST_TABLE;
        const uint32_t sel = ss == 0u ? td : ta, t = ss == 0u ? td : 2u + ta;
        if (!(ss == 0u && ah != 0u)) {  // a DC refinement reads raw bits only
          if (s.dht[t] == 0u) return ST_TABLE;  // selected, never defined
          e.tab[sel] = s.dht[t];
          e.tab_end[sel] = s.dht_end[t];
        }
        if (ss > 0u && s.coded[c][0] < 0) return ST_SCAN;  // AC before the component's first DC scan
        for (uint32_t k = ss; k <= se; ++k) {
          const int was = s.coded[c][k];
          if (ah == 0u ? was >= 0 : was != (int)ah) return ST_SCAN;  // first-coded twice; refined from a bit it does not stand at
          s.coded[c][k] = (int8_t)al;
        }
        e.comp[i] = (uint8_t)c;
        e.sel[i] = (uint8_t)sel;
        prev = c;
      }
      for (int i = ns; i < 3; ++i) e.comp[i] = e.sel[i] = 0;
      e.ns = (uint8_t)ns; e.ss = (uint8_t)ss; e.se = (uint8_t)se; e.ah = (uint8_t)ah; e.al = (uint8_t)al; e.level = 0;
      uint32_t units;
      if (ns == 1) {
        int bwc, bhc;
        own_blocks(H, W, e.comp[0], s.hs, s.vs, bwc, bhc);
        units = (uint32_t)bwc * (uint32_t)bhc;
      } else {
        units = (uint32_t)((W + 8 * s.hs - 1) / (8 * s.hs)) * (uint32_t)((H + 8 * s.vs - 1) / (8 * s.vs));
      }
      e.units = units;  // bounded by the call's H, W: <= 512 * 512
      e.ri = s.ri ? min(s.ri, units) : units;
      e.nint = (units + e.ri - 1u) / e.ri;
      e.start = send;
      e.end = flen;
      s.nscans += 1;
      s.pos = send;
      return ST_OK;
    }
    pos = send;
  }
}

__global__ __launch_bounds__(CS_JPGDEC_THREADS) void jpeg_progressive_kernel(CsJpgDecArgs a) {
  __shared__ __attribute__((aligned(16))) ProgLds s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = (int)rfl((uint32_t)(tid >> 6));
  const int img = blockIdx.x;
  if (a.status[img] != CS_JPGDEC_PENDING) return;  // a file of the other process, or one the baseline kernel has refused: uniform

  // the baseline kernel has checked the framing of the file's slot before it called the file pending
  const unsigned long long foff = a.file_offsets[img];
  const uint32_t flen = a.file_lengths[img];
  const bool framed = flen >= 4u && flen < (1u << 28) && foff <= a.files_bytes && (unsigned long long)flen <= a.files_bytes - foff;
  const uint8_t* file = a.files + (framed ? foff : 0ull);

  zigzag_to_lds(s.zz, tid);
  if (tid < 192) (&s.coded[0][0])[tid] = -1;
  if (tid < 4) { s.dht[tid] = 0u; s.dht_end[tid] = 0u; }
  if (tid == 0) {
    s.status = framed && file[0] == 0xFF && file[1] == 0xD8 ? ST_OK : ST_FRAMING;
    s.pos = 2u; s.ri = 0u; s.qdef = 0u;
    s.nc = 0; s.hs = 1; s.vs = 1; s.have_sof = 0; s.jfif = 0; s.nscans = 0; s.nlevels = 0; s.done = 0;
  }
  __syncthreads();

  // ---- the scan table: thread 0 from segment to segment, the workgroup over each scan's bytes.  At most 33 rounds.
  for (;;) {
    if (tid == 0 && s.status == ST_OK) s.status = walk(s, file, flen, a.H, a.W, a.levels);
    __syncthreads();
    if (s.status != ST_OK || s.done) break;  // uniform: LDS behind a barrier
    const int k = s.nscans - 1;
    const uint32_t nint = s.scan[k].nint, begin = s.scan[k].start;
    uint32_t* rst = a.scan_rst + ((unsigned long long)img * CS_JPGDEC_MAX_SCANS + (unsigned)k) * a.rst_slot;  // nint - 1 < rst_slot entries
    uint32_t scan_end = flen, count = 0;
    int misnumbered = 0;
    restart_positions(file, flen, begin, nint, rst, s.wcnt, s.wterm, tid, lane, wave, scan_end, count, misnumbered);
    if (misnumbered || count != nint - 1u) atomicCAS(&s.status, ST_OK, ST_RESTART);
    if (tid == 0) { s.scan[k].end = scan_end; s.pos = scan_end; }
    __syncthreads();
  }
  if (s.status != ST_OK) {  // uniform over the workgroup
    if (tid == 0) a.status[img] = (uint32_t)s.status;
    return;
  }

  const Geometry g = geometry(a.H, a.W, s.nc, s.hs, s.vs);
  int16_t* coef = a.coef + (unsigned long long)img * a.blocks_slot * 64ull;
  for (uint32_t i = (uint32_t)tid; i < g.nblocks * 8u; i += CS_JPGDEC_THREADS) reinterpret_cast<uint4*>(coef)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  // ---- the levels.  nscans, nlevels and the scan table stand since the last barrier above: every wave makes the same trips.
  {
    Bits r;
    r.file = file; r.flen = flen; r.win = s.inw[wave];
    const int nscans = s.nscans, nlevels = s.nlevels;
    int loaded = -1;  // the scan whose tables this wave's slice holds
    for (int level = 1; level <= nlevels; ++level) {
      uint32_t item = 0;
      for (int k = 0; k < nscans; ++k) {
        const ScanEnt& e = s.scan[k];
        if ((int)rfl(e.level) != level) continue;
        const uint32_t nint = rfl(e.nint), units = rfl(e.units), ri = rfl(e.ri);
        const int ns = (int)rfl(e.ns), ss = (int)rfl(e.ss), se = (int)rfl(e.se), ah = (int)rfl(e.ah), al = (int)rfl(e.al);
        const uint32_t* rst = a.scan_rst + ((unsigned long long)img * CS_JPGDEC_MAX_SCANS + (unsigned)k) * a.rst_slot;
        for (uint32_t j = ((uint32_t)wave - item) & 3u; j < nint; j += 4u) {
          if (rfl((uint32_t)*(volatile int*)&s.status) != 0u) break;  // some wave has ended the file
          int st = ST_OK;
          if (loaded != k && !(ss == 0 && ah != 0)) {  // this scan's tables into the wave's slice
            loaded = k;
            for (int t = 0; t < 2 && !st; ++t) {
              const uint32_t at = rfl(e.tab[t]), at_end = rfl(e.tab_end[t]);
              if (at == 0u) continue;
              const Huff h = huff_of(s, wave, t);
              wave_sync();
              for (int q = lane; q < (1 << CS_JPGDEC_PB); q += 64) h.look[q] = 0;
              uint32_t n = 0;
              int bad = 0;
              if (lane == 0) bad = huff_define(h, file, at, at_end, &n);
              bad = (int)rfl((uint32_t)bad);
              n = rfl(n);
              wave_sync();
              if (bad) { st = ST_TABLE; loaded = -1; break; }
              huff_fill_lookup(h, (int)n, lane, 64);
              wave_sync();
            }
          }
          const uint32_t from = j == 0u ? rfl(e.start) : rfl(rst[j - 1u]) + 2u;
          const uint32_t to = j + 1u < nint ? rfl(rst[j]) : rfl(e.end);
          if (!st) start_interval(r, min(from, flen), min(to, flen), lane);
          const uint32_t u1 = min(units, (j + 1u) * ri);
          uint32_t u = j * ri;

          if (st) {
          } else if (ss == 0) {  // ---- DC, first or refinement: blocks of one component in raster order, or MCUs
            int pred[3] = {0, 0, 0};
            int bwc = 1, bhc = 1;
            const int c0 = (int)rfl(e.comp[0]);
            own_blocks(a.H, a.W, c0, g.hs, g.vs, bwc, bhc);
            for (; u < u1 && !st; ++u) {
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                if (i >= ns || st) continue;
                const int c = (int)rfl(e.comp[i]);
                const int hc = ns > 1 && c == 0 ? g.hs : 1, vc = ns > 1 && c == 0 ? g.vs : 1;
                const Huff h = huff_of(s, wave, (int)rfl(e.sel[i]));
                for (int b = 0; b < hc * vc && !st; ++b) {
                  int by, bx;
                  if (ns == 1) { by = (int)(u / (uint32_t)bwc); bx = (int)(u % (uint32_t)bwc); }  // by < bhc <= bh[c], bx < bwc <= bw[c]
                  else { by = (int)(u / (uint32_t)g.mcux) * vc + b / hc; bx = (int)(u % (uint32_t)g.mcux) * hc + b % hc; }
                  int16_t* dc = coef + ((unsigned long long)first_of(g, c) + (unsigned long long)by * pitch_of(g, c) + (unsigned)bx) * 64ull;
                  if (r.nb < 32) refill(r, lane);
                  if (ah == 0) {
                    const int sym = decode_sym(h, r);
                    if (sym < 0) st = ST_CODE;
                    else if (sym > 11) st = ST_SYMBOL;
                    else if (sym) pred[i] += extend(take(r, sym), sym);
                    if (!st && lane == 0) dc[0] = (int16_t)(pred[i] * (1 << al));
                  } else if (take(r, 1)) {
                    if (lane == 0) dc[0] = (int16_t)(dc[0] | (1 << al));
                  }
                  if (r.nb < r.fake || (st && r.nb - 16 < r.fake)) st = ST_EXHAUSTED;  // an error read from the zeros behind the data is the data's end
                }
              }
            }
          } else {  // ---- AC: the blocks of one component in raster order
            const int c = (int)rfl(e.comp[0]);
            int bwc = 1, bhc = 1;
            own_blocks(a.H, a.W, c, g.hs, g.vs, bwc, bhc);
            const Huff h = huff_of(s, wave, (int)rfl(e.sel[0]));
            int16_t* plane = coef + (unsigned long long)first_of(g, c) * 64ull;
            const unsigned long long band = ((se == 63 ? 0ull : (1ull << (se + 1))) - 1ull) & ~((1ull << ss) - 1ull);  // bits ss .. se
            uint32_t eobrun = 0;
            if (ah == 0) {
              while (u < u1 && !st) {
                if (eobrun) {  // clipped to the blocks left in the interval
                  const uint32_t skip = min(eobrun, u1 - u);
                  u += skip;
                  eobrun -= skip;
                  continue;
                }
                int16_t* blk = own_block(plane, u, (uint32_t)bwc, pitch_of(g, c));
                int k2 = ss;
                while (k2 <= se) {
                  if (r.nb < 32) refill(r, lane);
                  const int sym = decode_sym(h, r);
                  if (sym < 0) { st = ST_CODE; break; }
                  const int run = sym >> 4, size = sym & 15;
                  if (size == 0) {
                    if (run == 15) { k2 += 16; continue; }
                    eobrun = 1u << run;
                    if (run) eobrun += take(r, run);
                    eobrun -= 1u;  // this block is the run's first
                    break;
                  }
                  k2 += run;
                  if (k2 > se || size > 10) { st = ST_SYMBOL; break; }
                  const int v = extend(take(r, size), size);
                  if (lane == 0) blk[k2] = (int16_t)(v * (1 << al));
                  k2 += 1;
                }
                if (r.nb < r.fake || (st && r.nb - 16 < r.fake)) st = ST_EXHAUSTED;
                u += 1;
              }
            } else {
              const int p1 = 1 << al;
              const uint32_t pitch = pitch_of(g, c);
              int next = u < u1 ? (int)own_block(plane, u, (uint32_t)bwc, pitch)[lane] : 0;
              for (; u < u1 && !st; ++u) {
                int16_t* blk = own_block(plane, u, (uint32_t)bwc, pitch);
                int v = next;
                if (u + 1u < u1) next = (int)own_block(plane, u + 1u, (uint32_t)bwc, pitch)[lane];  // in flight while this block is decoded
                const unsigned long long nz = __ballot(v != 0) & band;  // coefficients with a non-zero history
                unsigned long long corr = 0, fresh = 0, plus = 0;
                int k2 = ss;
                if (eobrun == 0u) {
                  while (k2 <= se) {
                    if (r.nb < 32) refill(r, lane);
                    const int sym = decode_sym(h, r);
                    if (sym < 0) { st = ST_CODE; break; }
                    int run = sym >> 4;
                    const int size = sym & 15;
                    int sign = 0;
                    if (size) {
                      if (size != 1) { st = ST_SYMBOL; break; }
                      sign = take(r, 1) ? 1 : -1;
                    } else if (run != 15) {
                      eobrun = 1u << run;
                      if (run) eobrun += take(r, run);
                      break;
                    }
                    while (k2 <= se) {  // past the non-zero coefficients, each with its correction bit, and `run` zero-history ones
                      if ((nz >> k2) & 1ull) {
                        if (r.nb < 32) refill(r, lane);
                        if (take(r, 1)) corr |= 1ull << k2;
                      } else if (--run < 0) {
                        break;
                      }
                      k2 += 1;
                    }
                    if (sign) {
                      if (k2 > se) { st = ST_SYMBOL; break; }  // the run leaves the band
                      fresh |= 1ull << k2;
                      if (sign > 0) plus |= 1ull << k2;
                    }
                    k2 += 1;
                  }
                }
                if (eobrun > 0u && !st) {  // inside an end-of-band run the rest of the band still takes its correction bits
                  for (; k2 <= se; ++k2) {
                    if ((nz >> k2) & 1ull) {
                      if (r.nb < 32) refill(r, lane);
                      if (take(r, 1)) corr |= 1ull << k2;
                    }
                  }
                  eobrun -= 1u;
                }
                if (r.nb < r.fake || (st && r.nb - 16 < r.fake)) st = ST_EXHAUSTED;
                if (!st && (corr | fresh)) {
                  if (((corr >> lane) & 1ull) && (v & p1) == 0) v += v >= 0 ? p1 : -p1;
                  if ((fresh >> lane) & 1ull) v = ((plus >> lane) & 1ull) ? p1 : -p1;
                  if ((band >> lane) & 1ull) blk[lane] = (int16_t)v;  // the band only: another wave may be at the block's other coefficients
                }
              }
            }
          }
          if (st && lane == 0) atomicCAS(&s.status, ST_OK, st);
        }
        item += nint;
      }
      __syncthreads();  // the level's coefficients stand before the next level reads them
    }
  }

  // ---- finish: times the quantiser, saturated, from zig-zag to natural order.  A wave takes a block: every lane's load is complete before any
  // lane's store is issued, because the store's value depends on the load.
  if (s.status == ST_OK) {
    for (uint32_t b = (uint32_t)wave; b < g.nblocks; b += 4u) {
      const int c = b < g.off[1] ? 0 : b < g.off[2] ? 1 : 2;
      const int v = coef[(unsigned long long)b * 64ull + (unsigned)lane];
      const int q = s.qt[s.tq[c]][lane];
      wave_sync();
      coef[(unsigned long long)b * 64ull + s.zz[lane]] = (int16_t)sat16(v * q);
    }
  }
  if (tid == 0) {
    a.status[img] = (uint32_t)s.status;
    uint32_t* info = a.info + 4ull * (unsigned)img;
    info[0] = (uint32_t)g.ncomp; info[1] = (uint32_t)g.hs; info[2] = (uint32_t)g.vs; info[3] = 0u;
  }
}

}  // namespace

hipError_t cs_jpgprog_launch(const CsJpgDecArgs& a, int I, hipStream_t st) {
  hipLaunchKernelGGL(jpeg_progressive_kernel, dim3(I), dim3(CS_JPGDEC_THREADS), 0, st, a);
  return hipGetLastError();
}
