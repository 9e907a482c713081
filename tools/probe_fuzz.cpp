// Stand-alone check of the host's file probes (crossscore_amd/csrc/jpeg_probe.h, png_probe.h) over untrusted bytes, for a CPU build under
// sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/probe_fuzz.cpp -o probe_fuzz
//   ./probe_fuzz a.jpg b.png c.jpg [mutations per file, default 4000]
//
// Each file goes to the probe its own (unmutated) signature names.  Every prefix of it and seeded mutations of it (byte flips, overwritten
// runs, spliced length fields, truncations) go through that probe.
// JPEG: each input once as cs_jpeg_probe walks it and once with CS_JPEG_PROBE_PROGRESSIVE, the walk of cs_jpeg_probe_ex that goes on through
// every scan of a progressive file to its EOI.  Baseline and progressive files may be mixed on the command line; for a progressive file the
// mutations land anywhere in the file, because that walk reads all of it.
// PNG: each input once without a span array and once with one of exactly the IDAT count the first walk reported, so that a span written past
// max_spans is a report too.  The mutations land anywhere in the file: the walk reads to IEND.
// Each input is copied into a heap block of exactly its own size, so a read at or beyond file + n is an AddressSanitizer report.  No GPU, no
// Python.  Exit status 0 and a summary line when nothing was reported.
#include "../crossscore_amd/csrc/jpeg_probe.h"
#include "../crossscore_amd/csrc/png_probe.h"

#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (unsigned)((g_state * 0x2545F4914F6CDD1Dull) >> 33);
}

static long g_counts[2][3];  // [jpeg, png][taken / bad framing / unsupported]

static void check(int rc, const cs_jpeg_probe_result& r, const cs_jpeg_probe_scans& x, size_t n) {
  if (rc < 0 || rc > 2) abort();
  if (rc == CS_JPEG_PROBE_OK && (r.entropy_offset >= n || r.sampling < 0 || r.sampling > 3 || r.width < 1 || r.width > 4096 || r.height < 1 || r.height > 4096)) abort();
  if (rc == CS_JPEG_PROBE_OK && (x.entropy_offset != r.entropy_offset || x.scans < 1 || x.scans > CS_JPEG_PROBE_MAX_SCANS || (x.process == 0 && x.scans != 1))) abort();
  if (rc != CS_JPEG_PROBE_OK && r.sampling != -1) abort();
  g_counts[0][rc] += 1;
}

static void run_jpeg(const uint8_t* exact, size_t n) {
  cs_jpeg_probe_result r, r0;
  cs_jpeg_probe_scans x, x0;
  char why[256], why0[256];
  const int rc = cs_jpeg_probe_walk(exact, n, &r, why, sizeof why);
  const int rc0 = cs_jpeg_probe_walk_ex(exact, n, 0, &r0, &x0, why0, sizeof why0);  // flags = 0 is the plain walk
  if (rc != rc0 || memcmp(&r, &r0, sizeof r) != 0 || (rc != CS_JPEG_PROBE_OK && strcmp(why, why0) != 0)) abort();
  check(rc0, r0, x0, n);
  const int rc1 = cs_jpeg_probe_walk_ex(exact, n, CS_JPEG_PROBE_PROGRESSIVE, &r, &x, why, sizeof why);
  check(rc1, r, x, n);
  if (rc0 == CS_JPEG_PROBE_OK && (rc1 != CS_JPEG_PROBE_OK || x.process != 0)) abort();  // what the plain walk takes, the flag does not lose
}

static void run_png(const uint8_t* exact, size_t n) {
  cs_png_info r, r1;
  char why[256], why1[256];
  const int rc = cs_png_probe_walk(exact, n, &r, nullptr, 0, why, sizeof why);
  if (rc < 0 || rc > 2) abort();
  if (rc == CS_OK ? (r.kind != CS_PNG_GRAY16 && r.kind != CS_PNG_RGB8) : r.kind != -1) abort();
  if (rc == CS_OK && (r.width < 1 || r.width > CS_PNG_MAX_SIDE || r.height < 1 || r.height > CS_PNG_MAX_SIDE || r.num_idat < 1 || r.interlace != 0)) abort();
  if (r.num_idat < 0 || (size_t)r.num_idat * 12 > n || r.idat_bytes > n) abort();
  g_counts[1][rc] += 1;
  // the second call of decode.probe_png: a span array of exactly num_idat entries (the redzone starts behind the last one)
  const size_t count = (size_t)r.num_idat;
  cs_png_span* spans = (cs_png_span*)malloc(count ? count * sizeof(cs_png_span) : 1);
  const int rc1 = cs_png_probe_walk(exact, n, &r1, spans, (int)count, why1, sizeof why1);
  if (rc1 != rc || memcmp(&r, &r1, sizeof r) != 0 || (rc != CS_OK && strcmp(why, why1) != 0)) abort();
  unsigned long long sum = 0;
  for (size_t i = 0; i < count; ++i) {  // every span the walk counted lies inside the file
    if (spans[i].offset < 8 || spans[i].offset > n || spans[i].length > n - spans[i].offset) abort();
    sum += spans[i].length;
  }
  if (sum != r.idat_bytes) abort();
  if (count > 1) {  // too little room: no write past max_spans, and a taken file says so
    const int rc2 = cs_png_probe_walk(exact, n, &r1, spans + 1, (int)count - 1, why1, sizeof why1);
    if (rc2 != (rc == CS_OK ? (int)CS_ERR_BAD_ARG : rc)) abort();
  }
  free(spans);
}

static void run(bool png, const std::vector<uint8_t>& bytes, size_t n) {
  uint8_t* exact = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: the redzone starts at file + n
  if (n) memcpy(exact, bytes.data(), n);
  if (png) run_png(exact, n);
  else run_jpeg(exact, n);
  free(exact);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg|file.png ... [mutations per file]\n", argv[0]);
    return 2;
  }
  int mutations = 4000, nfiles = argc - 1;
  if (argc > 2 && argv[argc - 1][0] >= '0' && argv[argc - 1][0] <= '9') {
    mutations = atoi(argv[argc - 1]);
    nfiles -= 1;
  }
  for (int f = 0; f < nfiles; ++f) {
    std::ifstream in(argv[1 + f], std::ios::binary);
    std::vector<uint8_t> good((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (good.size() < 4) {
      fprintf(stderr, "%s: cannot read\n", argv[1 + f]);
      return 2;
    }
    const bool png = memcmp(good.data(), "\x89PNG", 4) == 0;
    for (size_t n = 0; n <= good.size(); ++n) run(png, good, n);
    size_t header = good.size();  // what the walk reads of this file: all of a PNG and of a progressive JPEG
    char why[256];
    if (png) {
      cs_png_info r;  // (a PNG the probe refuses -- interlaced, palette -- is walked to its IEND all the same)
      if (cs_png_probe_walk(good.data(), good.size(), &r, nullptr, 0, why, sizeof why) == CS_ERR_BAD_ARG) {
        fprintf(stderr, "%s: the probe finds bad framing in the unmodified file: %s\n", argv[1 + f], why);
        return 2;
      }
    } else {
      cs_jpeg_probe_result r;
      cs_jpeg_probe_scans x;
      if (cs_jpeg_probe_walk_ex(good.data(), good.size(), CS_JPEG_PROBE_PROGRESSIVE, &r, &x, why, sizeof why) != CS_JPEG_PROBE_OK) {
        fprintf(stderr, "%s: the probe refuses the unmodified file: %s\n", argv[1 + f], why);
        return 2;
      }
      if (!x.process) header = (size_t)r.entropy_offset;
    }
    for (int k = 0; k < mutations; ++k) {
      std::vector<uint8_t> m = good;
      const int kind = (int)(rnd() % 5u);
      const int edits = 1 + (int)(rnd() % 4u);
      for (int e = 0; e < edits; ++e) {
        const size_t at = rnd() % header;
        if (kind == 0) m[at] ^= (uint8_t)(1u << (rnd() % 8u));
        else if (kind == 1) m[at] = (uint8_t)rnd();
        else if (kind == 2) { m[at] = 0xFF; if (at + 1 < m.size()) m[at + 1] = (uint8_t)(0xC0u + rnd() % 0x30u); }
        else if (kind == 3) { for (size_t j = at; j < m.size() && j < at + 1 + rnd() % 16u; ++j) m[j] = (uint8_t)rnd(); }
        else { if (at + 3 < m.size()) { m[at + 2] = (uint8_t)rnd(); m[at + 3] = (uint8_t)rnd(); } }
      }
      run(png, m, m.size());
      run(png, m, rnd() % (m.size() + 1));
      run(png, m, rnd() % (header + 1));
    }
  }
  printf("probe_fuzz:");
  for (int p = 0; p < 2; ++p)
    printf(" %s %ld inputs: %ld taken, %ld bad framing, %ld unsupported;", p ? "png" : "jpeg", g_counts[p][0] + g_counts[p][1] + g_counts[p][2],
           g_counts[p][0], g_counts[p][1], g_counts[p][2]);
  printf(" nothing reported\n");
  return 0;
}
