// Host-side differential checks of the shared Huffman decode core
// (csrc/jpeg_huff_core.h) and its packer (runtime/jpeg_huff_pack.cpp) against the
// host decoder (runtime/jpeg_entropy.cpp), built together under host
// AddressSanitizer + UndefinedBehaviorSanitizer.  For every file named on the
// command line it runs packer + core on
//   * the file itself (must be JPEG_OK),
//   * every prefix of it,
//   * the file with one byte replaced, at every 7th position, by a value from
//     a fixed LCG,
// with the image's byte span and coefficient span each copied to / decoded into
// an exactly sized heap allocation, so the sanitizers report one byte out of
// range.  Each run must give jpeg_decode's verdict (OK / the same refusal) and,
// where both are OK, identical coefficients.  Files named after --both-corrupt are
// decoded once and must be refused with JPEG_CORRUPT by both decoders.
// Build + run: tests/test_jpeg_huff_core_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../jpeg_huff_core.h"
#include "../runtime/jpeg_entropy.h"
#include "../runtime/jpeg_huff_pack.h"

using namespace idunno;

static int g_fail = 0;
static long g_both_ok = 0, g_both_corrupt = 0, g_refused = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

// packer + core on data[0, n) from its own exactly sized heap copy; returns the verdict
static int run_core(const uint8_t* data, size_t n, const char* what, size_t at, std::vector<int16_t>* coefs) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), data, n);
  const uint8_t* ptr = n ? in.get() : nullptr;
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b);
  coefs->clear();
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0, "%s@%zu: refused entry marked for the device\n", what, at);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  const char* why = jpeg_huff_check(b.desc.data(), 1, b.byte_total, (int64_t)b.sets.size(), b.coef_total);
  CHECK(why == nullptr, "%s@%zu: descriptor refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the core may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  std::unique_ptr<JpegHuffSet> set(new JpegHuffSet(b.sets[(size_t)d.set_idx]));
  const int st = jpeg_huff_decode_scan(d, span.get(), *set, out.get());
  coefs->assign(out.get(), out.get() + d.total_coefs);
  return st;
}

static void compare(const uint8_t* data, size_t n, const char* what, size_t at, bool must_ok) {
  std::vector<int16_t> got;
  const int st = run_core(data, n, what, at, &got);
  JpegHeader h;
  std::memset(&h, 0, sizeof(h));
  const int ps = jpeg_parse_header(n ? data : nullptr, n, &h);
  std::vector<int16_t> want(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(n ? data : nullptr, n, &h, want.data(), want.size());
  CHECK(st == hs, "%s@%zu: core %d, host decoder %d\n", what, at, st, hs);
  if (must_ok) CHECK(st == JPEG_OK, "%s: core status %d, expected ok\n", what, st);
  if (st == JPEG_OK && hs == JPEG_OK) {
    ++g_both_ok;
    CHECK(got == want, "%s@%zu: coefficients differ\n", what, at);
  } else if (st == JPEG_CORRUPT && hs == JPEG_CORRUPT && ps == JPEG_OK) {
    ++g_both_corrupt;                       // refused by the entropy stage itself
  } else {
    ++g_refused;
  }
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  std::FILE* f = std::fopen(path, "rb");
  if (f == nullptr) return false;
  uint8_t tmp[4096];
  size_t k;
  while ((k = std::fread(tmp, 1, sizeof(tmp), f)) > 0) out->insert(out->end(), tmp, tmp + k);
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: jpeg_huff_core_checks FILE.jpg...\n");
  long calls = 0;
  uint32_t lcg = 12345u;
  bool expect_corrupt = false;
  for (int a = 1; a < argc; ++a) {
    if (std::strcmp(argv[a], "--both-corrupt") == 0) {
      expect_corrupt = true;
      continue;
    }
    std::vector<uint8_t> d;
    if (!read_file(argv[a], &d) || d.empty()) {
      CHECK(false, "cannot read %s\n", argv[a]);
      continue;
    }
    if (expect_corrupt) {
      const long before = g_both_corrupt;
      compare(d.data(), d.size(), argv[a], d.size(), false);
      CHECK(g_both_corrupt == before + 1, "%s: expected both decoders to refuse it in the scan\n", argv[a]);
      ++calls;
      continue;
    }
    compare(d.data(), d.size(), argv[a], d.size(), true);
    ++calls;
    for (size_t n = 0; n < d.size(); ++n, ++calls) compare(d.data(), n, argv[a], n, false);
    for (size_t p = 0; p < d.size(); p += 7, ++calls) {
      lcg = lcg * 1664525u + 1013904223u;
      std::vector<uint8_t> m(d);
      m[p] = (uint8_t)(lcg >> 24);
      compare(m.data(), m.size(), "mutant", p, false);
    }
  }
  std::printf("both ok %ld, both corrupt in the scan %ld, refused by the parse %ld\n", g_both_ok, g_both_corrupt,
              g_refused);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
