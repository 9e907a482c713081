// Deflate code construction and the PNG filter arithmetic of png.hip's CS_PNG_DYNAMIC / CS_PNG_ADAPTIVE_FILTER paths.  Everything here is
// integer, serial over symbols (never over a segment's bytes) and __host__ __device__: the kernel calls it from one lane per code set, and a
// host program can run the same functions against zlib's inflate.
//
// A code set lives in one combined alphabet of 320 entries: literal/length symbols at [0, 288), distance symbols at [288, 320).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CS_HD __host__ __device__ __forceinline__
#else
#define CS_HD inline
#endif

namespace cs_huff {

constexpr int kLL = 288, kD = 32, kAlpha = kLL + kD;
constexpr int kHdrWords = 80;  // 14 + 19 * 3 + 316 * 7 = 2283 bits at most

// length 3 .. 258 -> length symbol 257 .. 285, its extra-bit count and value (RFC 1951 3.2.5)
CS_HD void length_symbol(int len, uint32_t* sym, uint32_t* eb, uint32_t* ev) {
  *eb = 0; *ev = 0;
  if (len <= 10) { *sym = 254u + (uint32_t)len; return; }
  if (len == 258) { *sym = 285u; return; }
  const uint32_t l = (uint32_t)len - 3u;
  const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
  *sym = 261u + 4u * e + ((l >> e) & 3u);
  *eb = e;
  *ev = l & ((1u << e) - 1u);
}

// distance 1 .. 32768 -> distance code 0 .. 29, its extra-bit count and value
CS_HD void dist_symbol(int dist, uint32_t* dc, uint32_t* db, uint32_t* dv) {
  *db = 0; *dv = 0;
  if (dist <= 4) { *dc = (uint32_t)dist - 1u; return; }
  const uint32_t d = (uint32_t)dist - 1u;
  const uint32_t b = (31u - (uint32_t)__builtin_clz(d)) - 1u;
  *dc = 2u * b + 2u + ((d >> b) & 1u);
  *db = b;
  *dv = d & ((1u << b) - 1u);
}

// extra bits behind entry t of the combined alphabet
CS_HD uint32_t extra_bits(int t) {
  if (t < 265) return 0u;
  if (t < 285) return (uint32_t)(t - 261) >> 2;
  if (t < kLL + 4) return 0u;
  if (t < kLL + 30) return (uint32_t)((t - kLL) >> 1) - 1u;
  return 0u;
}

// code length of entry t in the fixed code of RFC 1951 3.2.6
CS_HD uint32_t fixed_length(int t) { return t < 144 ? 8u : t < 256 ? 9u : t < 280 ? 7u : t < kLL ? 8u : 5u; }

// rank of symbol t among the used symbols of hist[lo, hi), ascending by (count, symbol); *used = how many are used.  t itself must be used.
CS_HD int sort_rank(const uint32_t* hist, int lo, int hi, int t, int* used) {
  const uint32_t f = hist[t];
  int r = 0, m = 0;
  for (int u = lo; u < hi; ++u) {
    const uint32_t h = hist[u];
    m += h != 0u;
    r += h != 0u && (h < f || (h == f && u < t));
  }
  *used = m;
  return r;
}

// Length-limited prefix code lengths.  key[0, m): the used symbols' counts, ascending with ties by symbol index; sym[0, m): their entries in
// len[], which the caller has zeroed; num: 16 words of scratch.  m == 0 leaves len alone; m == 1 gives the symbol and one unused neighbour
// (entry `base` or base + 1) one bit each, a complete code every inflate takes.  Otherwise: the in-place minimum-redundancy construction of
// Moffat and Katajainen (1995) over the sorted counts, then depths above maxbits are folded to maxbits and the Kraft sum is brought back to
// exactly 1 by lengthening the shallowest codes that can give way (each step removes 2^-maxbits); the rarest symbols get the longest codes.
CS_HD void code_lengths(uint32_t* key, const uint16_t* sym, int m, int base, int maxbits, uint32_t* num, uint8_t* len) {
  if (m == 0) return;
  if (m == 1) {
    len[sym[0]] = 1;
    len[sym[0] == base ? base + 1 : base] = 1;
    return;
  }
  key[0] += key[1];
  int root = 0, leaf = 2, next;
  for (next = 1; next < m - 1; ++next) {
    if (leaf >= m || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = (uint32_t)next; }
    else key[next] = key[leaf++];
    if (leaf >= m || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = (uint32_t)next; }
    else key[next] += key[leaf++];
  }
  key[m - 2] = 0;
  for (next = m - 3; next >= 0; --next) key[next] = key[key[next]] + 1u;
  int avbl = 1, used = 0;
  uint32_t dpth = 0;
  root = m - 2; next = m - 1;
  while (avbl > 0) {
    while (root >= 0 && key[root] == dpth) { ++used; --root; }
    while (avbl > used) { key[next--] = dpth; --avbl; }
    avbl = 2 * used; ++dpth; used = 0;
  }
  // key[k] is now the depth of the k-th symbol
  for (int l = 0; l <= maxbits; ++l) num[l] = 0;
  for (int k = 0; k < m; ++k) num[key[k] < (uint32_t)maxbits ? key[k] : (uint32_t)maxbits] += 1u;
  uint32_t total = 0;
  for (int l = maxbits; l >= 1; --l) total += num[l] << (maxbits - l);
  while (total > (1u << maxbits)) {
    num[maxbits] -= 1u;
    for (int l = maxbits - 1; l >= 1; --l)
      if (num[l]) { num[l] -= 1u; num[l + 1] += 2u; break; }
    total -= 1u;
  }
  int k = m;
  for (int l = 1; l <= maxbits; ++l)
    for (uint32_t c = 0; c < num[l]; ++c) len[sym[--k]] = (uint8_t)l;
}

// canonical codes of len[0, n), bit-reversed for the LSB-first stream; next: 16 words of scratch
CS_HD void canonical_codes(const uint8_t* len, int n, int maxbits, uint32_t* next, uint16_t* code) {
  for (int l = 0; l <= maxbits; ++l) next[l] = 0;
  for (int s = 0; s < n; ++s) next[len[s]] += 1u;
  uint32_t c = 0, prev = 0;
  next[0] = 0;
  for (int l = 1; l <= maxbits; ++l) { c = (c + prev) << 1; prev = next[l]; next[l] = c; }
  for (int s = 0; s < n; ++s) {
    const int l = len[s];
    uint32_t r = 0;
    if (l) {
      uint32_t v = next[l]++;
      for (int b = 0; b < l; ++b) { r = (r << 1) | (v & 1u); v >>= 1; }
    }
    code[s] = (uint16_t)r;
  }
}

struct HeaderScratch {
  uint16_t seq[kAlpha];  // code-length symbol | extra value << 8
  uint32_t key[19];
  uint16_t sym[19];
  uint16_t code[19];
  uint8_t len[20];
  uint32_t freq[19];
  uint32_t num[16];
};

CS_HD void put_bits(uint32_t* w, uint32_t* pos, uint32_t v, uint32_t n) {
  const uint32_t p = *pos, sh = p & 31u;
  w[p >> 5] |= v << sh;
  if (sh + n > 32u) w[(p >> 5) + 1] |= v >> (32u - sh);
  *pos = p + n;
}

// The header of a dynamic block behind its three BFINAL / BTYPE bits (RFC 1951 3.2.7): HLIT, HDIST, HCLEN, the code-length code, then the
// lengths of len[0, 288) and len[288, 320) as one sequence with zero runs as symbols 17 / 18 (16 is not used).  hdr: kHdrWords words, zeroed
// here; returns the bit count.
CS_HD uint32_t dynamic_header(const uint8_t* len, HeaderScratch* s, uint32_t* hdr) {
  int hlit = 286, hdist = 30;
  while (hlit > 257 && len[hlit - 1] == 0) --hlit;
  while (hdist > 1 && len[kLL + hdist - 1] == 0) --hdist;
  const int total = hlit + hdist;
  for (int k = 0; k < 19; ++k) { s->freq[k] = 0; s->len[k] = 0; }
  int nseq = 0;
  for (int i = 0; i < total;) {
    const uint32_t v = len[i < hlit ? i : kLL + (i - hlit)];
    int run = 1;
    uint32_t item = v;
    if (v == 0) {
      while (i + run < total && run < 138) {
        const int j = i + run;
        if (len[j < hlit ? j : kLL + (j - hlit)] != 0) break;
        ++run;
      }
      if (run >= 11) item = 18u | ((uint32_t)(run - 11) << 8);
      else if (run >= 3) item = 17u | ((uint32_t)(run - 3) << 8);
      else run = 1;
    }
    s->seq[nseq++] = (uint16_t)item;
    s->freq[item & 0xffu] += 1u;
    i += run;
  }
  int m = 0;  // the used code-length symbols, ascending by (count, symbol)
  for (int k = 0; k < 19; ++k) {
    const uint32_t f = s->freq[k];
    if (!f) continue;
    int p = m++;
    while (p > 0 && s->key[p - 1] > f) { s->key[p] = s->key[p - 1]; s->sym[p] = s->sym[p - 1]; --p; }
    s->key[p] = f; s->sym[p] = (uint16_t)k;
  }
  code_lengths(s->key, s->sym, m, 0, 7, s->num, s->len);
  canonical_codes(s->len, 19, 7, s->num, s->code);
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 19;
  while (hclen > 4 && s->len[order[hclen - 1]] == 0) --hclen;
  for (int w = 0; w < kHdrWords; ++w) hdr[w] = 0;
  uint32_t pos = 0;
  put_bits(hdr, &pos, (uint32_t)(hlit - 257), 5);
  put_bits(hdr, &pos, (uint32_t)(hdist - 1), 5);
  put_bits(hdr, &pos, (uint32_t)(hclen - 4), 4);
  for (int k = 0; k < hclen; ++k) put_bits(hdr, &pos, s->len[order[k]], 3);
  for (int k = 0; k < nseq; ++k) {
    const uint32_t item = s->seq[k], c = item & 0xffu;
    put_bits(hdr, &pos, s->code[c], s->len[c]);
    if (c == 17u) put_bits(hdr, &pos, item >> 8, 3);
    else if (c == 18u) put_bits(hdr, &pos, item >> 8, 7);
  }
  return pos;
}

// ---- PNG filters (PNG specification, section 9): x the byte, a left, b above, c above-left
CS_HD uint32_t paeth_predictor(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
  pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

CS_HD uint32_t png_filter(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) pred = paeth_predictor(a, b, c);
  return (x - pred) & 0xffu;
}

}  // namespace cs_huff
