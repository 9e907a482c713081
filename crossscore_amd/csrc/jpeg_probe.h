// The host's walk over a JPEG file's marker segments (cs_jpeg_probe, cs_jpeg_probe_ex): plain C++ over untrusted bytes, no device and no HIP,
// so that it also builds into a stand-alone program under sanitizers (tools/probe_fuzz.cpp).  It never reads at or beyond file + n.
//
// Without CS_JPEG_PROBE_PROGRESSIVE the walk ends at the SOS of a baseline file.  With it a SOF2 file is walked to its EOI: every scan is
// checked against T.81 G.1.1.1.1 (what libjpeg only warns about is refused here) and the progression has to be complete, because an incomplete
// one is where libjpeg's block smoothing starts.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

enum { CS_JPEG_PROBE_OK = 0, CS_JPEG_PROBE_BAD_ARG = 1, CS_JPEG_PROBE_UNSUPPORTED = 2 };  // CS_OK / CS_ERR_BAD_ARG / CS_ERR_UNSUPPORTED

enum { CS_JPEG_PROBE_PROGRESSIVE = 1 };                                                   // CS_JPEG_PROGRESSIVE
enum { CS_JPEG_PROBE_MAX_SCANS = 32 };

struct cs_jpeg_probe_result {
  int width, height, components, sampling, restart_interval;  // sampling: 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0 (CS_JPEG_*)
  unsigned long long entropy_offset;
};

struct cs_jpeg_probe_scans {  // cs_jpeg_scan_info
  int process, scans;         // process: 0 baseline, 1 progressive
  unsigned long long entropy_offset;  // the first scan's data
};

#define CS_JPEG_PROBE_FAIL(code, ...) (snprintf(err, err_len, __VA_ARGS__), (code))

// Fills *out (sampling -1 until the file is known to be taken) and returns one of CS_JPEG_PROBE_*; on failure err holds the reason.
static inline int cs_jpeg_probe_walk_ex(const uint8_t* file, size_t n, int flags, cs_jpeg_probe_result* out, cs_jpeg_probe_scans* ext, char* err,
                                        size_t err_len) {
  memset(out, 0, sizeof *out);
  memset(ext, 0, sizeof *ext);
  out->sampling = -1;
  static const uint8_t soi[2] = {0xFF, 0xD8};
  if (memcmp(file, soi, n < 2 ? n : 2) != 0) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: not a JPEG file (no SOI marker)");
  if (n < 2) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: %zu bytes end inside the SOI marker", n);
  if (n >= ((size_t)1 << 28)) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a file of %zu bytes is above the decoder's 256 MiB", n);
  size_t pos = 2;
  bool have_sof = false, jfif = false;
  int nc = 0, hv0 = 0x11;
  unsigned id[3] = {0, 0, 0};
  bool progressive = false;
  int scans = 0;
  signed char coded[3][64];  // per coefficient the Al it was last coded with, -1 before its first scan
  memset(coded, -1, sizeof coded);
  for (;;) {
    if (scans > 0 && n - pos >= 2 && file[pos] == 0xFF && file[pos + 1] == 0xD9) {  // EOI of a progressive file
      for (int c = 0; c < nc; ++c)
        for (int k = 0; k < 64; ++k)
          if (coded[c][k] != 0)
            return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: incomplete progression: coefficient %d of component %d %s (block smoothing is not built)",
                                      k, c, coded[c][k] < 0 ? "is never coded" : "stops above bit 0");
      ext->process = 1;
      ext->scans = scans;
      out->sampling = nc == 1 ? 0 : hv0 == 0x11 ? 1 : hv0 == 0x21 ? 2 : 3;
      return CS_JPEG_PROBE_OK;
    }
    if (scans > 0 && n - pos < 4)
      return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the progressive file ends at byte %zu after %d scans without an EOI marker", pos, scans);
    if (n - pos < 4) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: the file ends inside a segment's framing at byte %zu (no SOS)", pos);
    if (file[pos] != 0xFF) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: byte %zu is %02x where a marker must begin", pos, file[pos]);
    const unsigned m = file[pos + 1];
    if (m == 0xFF) { pos += 1; continue; }  // a fill byte
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9))
      return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: marker FF%02X at byte %zu before the scan", m, pos);
    const size_t len = ((size_t)file[pos + 2] << 8) | file[pos + 3];
    if (len < 2 || len > n - pos - 2)
      return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: the segment at byte %zu is %zu bytes long and runs past the file's end", pos, len);
    const uint8_t* seg = file + pos + 4;
    const size_t body = len - 2;
    if (m == 0xC0 || (m == 0xC2 && (flags & CS_JPEG_PROBE_PROGRESSIVE))) {
      progressive = m == 0xC2;
      if (have_sof || body < 6) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: a second or short SOF0 segment at byte %zu", pos);
      nc = seg[5];
      if (body != 6 + 3 * (size_t)nc) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: SOF0 of %zu bytes for %d components", len, nc);
      out->height = (seg[1] << 8) | seg[2];
      out->width = (seg[3] << 8) | seg[4];
      out->components = nc;
      if (seg[0] != 8) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: %d-bit samples (8 only)", seg[0]);
      if (nc != 1 && nc != 3) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: %d components (1 or 3)", nc);
      for (int c = 0; c < nc; ++c) {
        id[c] = seg[6 + 3 * c];
        const int hv = seg[7 + 3 * c];
        if (c == 0) hv0 = hv;
        if (c > 0 ? hv != 0x11 : (hv != 0x11 && (nc == 1 || (hv != 0x21 && hv != 0x22))))
          return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: component %d samples %d x %d (gray 1x1; colour 4:4:4, 4:2:2, 4:2:0)", c, hv >> 4, hv & 15);
        if (seg[8 + 3 * c] > 3) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: quantisation table %d", seg[8 + 3 * c]);
      }
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: marker FF%02X: only baseline (SOF0) files are decoded on the device", m);
    } else if (m == 0xC4) {
      for (size_t p = 0; p < body;) {
        if ((seg[p] >> 4) > 1 || (seg[p] & 15) > 1) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: Huffman table class %d id %d (baseline: 0 / 1)", seg[p] >> 4, seg[p] & 15);
        if (body - p < 17) break;  // the device says what is wrong with the table
        size_t total = 0;
        for (int l = 1; l <= 16; ++l) total += seg[p + l];
        p += 17 + total;
      }
    } else if (m == 0xDB) {
      if (scans > 0) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a DQT segment at byte %zu behind the first scan", pos);
      for (size_t p = 0; p < body; p += 65)
        if (seg[p] >> 4) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: 16-bit quantisation table");
    } else if (m == 0xDD) {
      if (scans > 0) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a DRI segment at byte %zu behind the first scan", pos);
      if (body != 2) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: DRI segment of %zu bytes", len);
      out->restart_interval = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0) {
      if (body >= 5 && memcmp(seg, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (body >= 5 && memcmp(seg, "Adobe", 5) == 0) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a file with an Adobe APP14 segment");
    } else if (m == 0xDA) {
      if (!have_sof) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: SOS at byte %zu before any SOF", pos);
      if (body < 1 || body != 4 + 2 * (size_t)seg[0]) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: SOS of %zu bytes", len);
      const int ns = seg[0];
      if (progressive) {
        if (scans == 0) {  // the frame-level rules of the baseline walk
          if (nc == 3 && !jfif && !(id[0] == 1 && id[1] == 2 && id[2] == 3))
            return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: three components without JFIF and with ids other than 1, 2, 3: colour space unknown");
          if (out->height < 1 || out->width < 1 || out->height > 4096 || out->width > 4096)
            return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: %d x %d is outside 1 .. 4096", out->height, out->width);
          if (hv0 != 0x11 && out->width <= 4)
            return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a subsampled file %d wide (libjpeg's replication upsampler below 5 is not built)", out->width);
        }
        if (scans == CS_JPEG_PROBE_MAX_SCANS) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: more than %d scans", CS_JPEG_PROBE_MAX_SCANS);
        if (ns < 1 || ns > nc) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d names %d of the %d components", scans + 1, ns, nc);
        int comp[3] = {0, 0, 0}, prev = -1;
        for (int i = 0; i < ns; ++i) {
          int c = prev + 1;
          while (c < nc && id[c] != seg[1 + 2 * i]) ++c;
          if (c >= nc) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the components of scan %d are not a subset of the frame's, in order", scans + 1);
          if ((seg[2 + 2 * i] >> 4) > 1 || (seg[2 + 2 * i] & 15) > 1) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the scan selects Huffman table %02x", seg[2 + 2 * i]);
          comp[i] = prev = c;
        }
        const int ss = seg[1 + 2 * ns], se = seg[2 + 2 * ns], ah = seg[3 + 2 * ns] >> 4, al = seg[3 + 2 * ns] & 15;
        if (ss == 0 ? se != 0 : (ns != 1 || ss > se || se > 63))
          return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d: band %d .. %d of %d components (a DC scan is 0 .. 0; an AC scan has one component and 1 <= Ss <= Se <= 63)",
                                    scans + 1, ss, se, ns);
        if (al > 13) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d: Al = %d (13 at most)", scans + 1, al);
        if (ah != 0 && ah != al + 1) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d: Ah = %d beside Al = %d (a refinement has Ah = Al + 1)", scans + 1, ah, al);
        for (int i = 0; i < ns; ++i) {
          if (ss > 0 && coded[comp[i]][0] < 0)
            return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d: AC coefficients of component %d before its first DC scan", scans + 1, comp[i]);
          for (int k = ss; k <= se; ++k) {
            const int was = coded[comp[i]][k];
            if (ah == 0 && was >= 0)
              return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d codes coefficient %d of component %d for the first time again", scans + 1, k, comp[i]);
            if (ah != 0 && was != ah)
              return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: scan %d refines coefficient %d of component %d from bit %d, which %s", scans + 1, k, comp[i],
                                        ah, was < 0 ? "was never coded" : "is not where it stands");
            coded[comp[i]][k] = (signed char)al;
          }
        }
        const size_t data = pos + 2 + len;
        if (data >= n) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: the file ends with its SOS segment (no entropy-coded data)");
        if (scans == 0) out->entropy_offset = ext->entropy_offset = data;
        scans += 1;
        // the scan's data: on to the next marker that is neither a stuffed FF00, a fill FF nor RSTn
        size_t p = data;
        while (p < n) {
          const uint8_t* ff = (const uint8_t*)memchr(file + p, 0xFF, n - p);
          if (!ff) { p = n; break; }
          p = (size_t)(ff - file);
          if (p + 1 >= n) { p = n; break; }
          const unsigned b = file[p + 1];
          if (b == 0xFF) p += 1;
          else if (b == 0x00 || (b >= 0xD0 && b <= 0xD7)) p += 2;
          else break;
        }
        if (p >= n) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the data of scan %d runs to the file's end (no EOI marker)", scans);
        pos = p;
        continue;
      }
      if (ns != nc) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a scan of %d of the %d components (one interleaved scan only)", ns, nc);
      for (int c = 0; c < nc; ++c) {
        if (seg[1 + 2 * c] != id[c]) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the scan's components are not the frame's, in order");
        if ((seg[2 + 2 * c] >> 4) > 1 || (seg[2 + 2 * c] & 15) > 1) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: the scan selects Huffman table %02x", seg[2 + 2 * c]);
      }
      if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0)
        return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: spectral selection / approximation of a non-baseline scan");
      if (nc == 3 && !jfif && !(id[0] == 1 && id[1] == 2 && id[2] == 3))
        return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: three components without JFIF and with ids other than 1, 2, 3: colour space unknown");
      if (out->height < 1 || out->width < 1 || out->height > 4096 || out->width > 4096)
        return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: %d x %d is outside 1 .. 4096", out->height, out->width);
      if (hv0 != 0x11 && out->width <= 4)
        return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_UNSUPPORTED, "jpeg_probe: a subsampled file %d wide (libjpeg's replication upsampler below 5 is not built)", out->width);
      out->entropy_offset = ext->entropy_offset = pos + 2 + len;
      if (out->entropy_offset >= n) return CS_JPEG_PROBE_FAIL(CS_JPEG_PROBE_BAD_ARG, "jpeg_probe: the file ends with its SOS segment (no entropy-coded data)");
      out->sampling = nc == 1 ? 0 : hv0 == 0x11 ? 1 : hv0 == 0x21 ? 2 : 3;
      ext->scans = 1;
      return CS_JPEG_PROBE_OK;
    }
    pos += 2 + len;
  }
}

static inline int cs_jpeg_probe_walk(const uint8_t* file, size_t n, cs_jpeg_probe_result* out, char* err, size_t err_len) {
  cs_jpeg_probe_scans ext;
  return cs_jpeg_probe_walk_ex(file, n, 0, out, &ext, err, err_len);
}
