// Stand-alone check of the host's JPEG probe (crossscore_amd/csrc/jpeg_probe.h) over untrusted bytes, for a CPU build under sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_probe_fuzz.cpp -o jpeg_probe_fuzz
//   ./jpeg_probe_fuzz a.jpg b.jpg c.jpg [mutations per file, default 4000]
//
// Every prefix of each file and seeded mutations of it (byte flips, overwritten runs, spliced length fields, truncations) go through the probe,
// each input once as cs_jpeg_probe walks it and once with CS_JPEG_PROBE_PROGRESSIVE, the walk of cs_jpeg_probe_ex that goes on through every
// scan of a progressive file to its EOI.  Baseline and progressive files may be mixed on the command line; for a progressive file the
// mutations land anywhere in the file, because that walk reads all of it.
// Each input is copied into a heap block of exactly its own size, so a read at or beyond file + n is an AddressSanitizer report.  No GPU, no
// Python.  Exit status 0 and a summary line when nothing was reported.
#include "../crossscore_amd/csrc/jpeg_probe.h"

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

static long g_counts[3];

static void check(int rc, const cs_jpeg_probe_result& r, const cs_jpeg_probe_scans& x, size_t n) {
  if (rc < 0 || rc > 2) abort();
  if (rc == CS_JPEG_PROBE_OK && (r.entropy_offset >= n || r.sampling < 0 || r.sampling > 3 || r.width < 1 || r.width > 4096 || r.height < 1 || r.height > 4096)) abort();
  if (rc == CS_JPEG_PROBE_OK && (x.entropy_offset != r.entropy_offset || x.scans < 1 || x.scans > CS_JPEG_PROBE_MAX_SCANS || (x.process == 0 && x.scans != 1))) abort();
  if (rc != CS_JPEG_PROBE_OK && r.sampling != -1) abort();
  g_counts[rc] += 1;
}

static void run(const std::vector<uint8_t>& bytes, size_t n) {
  uint8_t* exact = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: the redzone starts at file + n
  if (n) memcpy(exact, bytes.data(), n);
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
  free(exact);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ... [mutations per file]\n", argv[0]);
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
    for (size_t n = 0; n <= good.size(); ++n) run(good, n);
    cs_jpeg_probe_result r;
    cs_jpeg_probe_scans x;
    char why[256];
    if (cs_jpeg_probe_walk_ex(good.data(), good.size(), CS_JPEG_PROBE_PROGRESSIVE, &r, &x, why, sizeof why) != CS_JPEG_PROBE_OK) {
      fprintf(stderr, "%s: the probe refuses the unmodified file: %s\n", argv[1 + f], why);
      return 2;
    }
    const size_t header = x.process ? good.size() : (size_t)r.entropy_offset;  // what the walk reads of this file
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
      run(m, m.size());
      run(m, rnd() % (m.size() + 1));
      run(m, rnd() % (header + 1));
    }
  }
  printf("jpeg_probe_fuzz: %ld inputs: %ld taken, %ld bad framing, %ld unsupported; nothing reported\n", g_counts[0] + g_counts[1] + g_counts[2],
         g_counts[0], g_counts[1], g_counts[2]);
  return 0;
}
