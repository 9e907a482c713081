// The host's walk over a PNG file's chunks (cs_png_probe): plain C++ over untrusted bytes, no device and no HIP, so that it also builds into a
// stand-alone program under sanitizers (tools/probe_fuzz.cpp).  It never reads at or beyond file + n and writes at most max_spans spans.
#pragma once

#include <cstdio>
#include <cstring>

#include "../../include/crossscore_hip.h"  // plain C: cs_png_info, cs_png_span, CS_PNG_GRAY16 / CS_PNG_RGB8, CS_OK / CS_ERR_*

enum { CS_PNG_MAX_SIDE = 4096 };  // the encoder's and both decoders' largest H and W

#define CS_PNG_PROBE_FAIL(code, ...) (snprintf(err, err_len, __VA_ARGS__), (code))

// Fills *out (kind -1 unless the file is taken) and, with spans, the first max_spans IDAT spans; returns CS_OK, CS_ERR_BAD_ARG or
// CS_ERR_UNSUPPORTED; on failure err holds the reason.
static inline int cs_png_probe_walk(const uint8_t* file, size_t n, cs_png_info* out, cs_png_span* spans, int max_spans, char* err,
                                    size_t err_len) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  memset(out, 0, sizeof *out);
  out->kind = -1;
  if (memcmp(file, sig, n < 8 ? n : 8) != 0) return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: not a PNG file (no PNG signature)");
  if (n < 8) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: %zu bytes end inside the PNG signature", n);
  if (n >= ((size_t)1 << 28)) return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: a file of %zu bytes is above the decoder's 256 MiB", n);
  auto be = [&](size_t p) { return ((uint32_t)file[p] << 24) | ((uint32_t)file[p + 1] << 16) | ((uint32_t)file[p + 2] << 8) | file[p + 3]; };
  size_t pos = 8;
  int count = 0;
  bool have_ihdr = false, have_end = false;
  unsigned long long idat_bytes = 0;
  while (!have_end) {
    if (n - pos < 12) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: the file ends inside a chunk's framing at byte %zu (no IEND)", pos);
    const uint32_t len = be(pos);
    if (len > n - pos - 12) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: the chunk at byte %zu is %u bytes long and runs past the file's end", pos, len);
    const uint8_t* t = file + pos + 4;
    if (!have_ihdr) {
      if (memcmp(t, "IHDR", 4) != 0 || len != 13) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: the first chunk is not a 13-byte IHDR");
      have_ihdr = true;
      out->width = (int)be(pos + 8);
      out->height = (int)be(pos + 12);
      if (be(pos + 8) == 0 || be(pos + 12) == 0 || be(pos + 8) > 0x7fffffffu || be(pos + 12) > 0x7fffffffu) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: IHDR size 0 or above 2^31 - 1");
      out->bit_depth = file[pos + 16];
      out->color_type = file[pos + 17];
      out->interlace = file[pos + 20];
      if (file[pos + 18] != 0 || file[pos + 19] != 0) return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: compression / filter method %d / %d", file[pos + 18], file[pos + 19]);
    } else if (memcmp(t, "IDAT", 4) == 0) {
      if (spans && count < max_spans) { spans[count].offset = (uint32_t)(pos + 8); spans[count].length = len; }
      count += 1;
      idat_bytes += len;
    } else if (memcmp(t, "IEND", 4) == 0) {
      have_end = true;
    } else if (memcmp(t, "PLTE", 4) != 0 && !(t[0] & 0x20)) {
      return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: unknown critical chunk %.4s", (const char*)t);
    }
    pos += 12 + (size_t)len;
  }
  out->num_idat = count;
  out->idat_bytes = idat_bytes;
  if (count == 0) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: no IDAT chunk");
  if (out->interlace != 0) return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: interlaced files are not decoded on the device");
  const int ct = out->color_type, d = out->bit_depth;
  if (!((d == 8 && (ct == 2 || ct == 6 || ct == 0)) || (d == 16 && ct == 0)))
    return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: colour type %d with bit depth %d is not decoded on the device (8-bit gray / RGB / RGBA, 16-bit gray)", ct, d);
  if (out->height > CS_PNG_MAX_SIDE || out->width > CS_PNG_MAX_SIDE)
    return CS_PNG_PROBE_FAIL(CS_ERR_UNSUPPORTED, "png_probe: %d x %d is larger than %d x %d", out->height, out->width, CS_PNG_MAX_SIDE, CS_PNG_MAX_SIDE);
  out->kind = d == 16 ? CS_PNG_GRAY16 : CS_PNG_RGB8;
  if (spans && count > max_spans) return CS_PNG_PROBE_FAIL(CS_ERR_BAD_ARG, "png_probe: %d IDAT chunks, room for %d spans", count, max_spans);
  return CS_OK;
}
