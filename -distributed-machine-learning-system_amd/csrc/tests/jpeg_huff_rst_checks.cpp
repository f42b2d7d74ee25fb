// Host-side differential checks of the restart-interval Huffman decode
// (csrc/jpeg_huff_rst.h) and its packer layout (runtime/jpeg_huff_pack.cpp with
// restart_intervals) against the host decoder (runtime/jpeg_entropy.cpp), built
// together under host AddressSanitizer + UndefinedBehaviorSanitizer.
//
// For every file named on the command line it decodes
//   * the file itself (must be JPEG_OK),
//   * every prefix of it,
//   * the file with every 7th byte replaced in turn by FF, by 00 and by its value
//     XOR 55.
// Each input is planned with restart_intervals, its word span and coefficient span
// in exactly sized heap allocations.  A gpu == 4 entry goes through
// jpeg_huff_rst_check and then has every item decoded by jpeg_huff_decode_interval,
// once in ascending and once in descending item order, each into a fresh zeroed
// span; the verdict is the maximum over the items, as the kernel's atomicMax makes
// it.  A gpu == 1 entry is decoded by jpeg_huff_decode_scan.  Each run must give
// jpeg_decode's verdict and, where both are OK, identical coefficients; the two item
// orders must give identical coefficients whatever the verdict.
// Build + run: tests/test_jpeg_huff_rst_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../jpeg_huff_core.h"
#include "../jpeg_huff_rst.h"
#include "../runtime/jpeg_entropy.h"
#include "../runtime/jpeg_huff_pack.h"

using namespace idunno;

static int g_fail = 0;
static long g_rst_ok = 0, g_rst_corrupt = 0, g_lane_ok = 0, g_lane_corrupt = 0, g_refused = 0, g_items = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

// packer + the lanes of the interval kernel, one after the other, on data[0, n); returns the verdict
// (the parse's when it refuses) and whether the interval path took the input
static int run_rst(const uint8_t* ptr, size_t n, bool descending, const char* what, size_t at,
                   std::vector<int16_t>* coefs, bool* intervals) {
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  JpegOptions opt;
  opt.restart_intervals = true;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, 0, opt);
  coefs->clear();
  *intervals = false;
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0 && b.rst_items.empty(), "%s@%zu: refused entry marked for the device\n", what, at);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  const char* why = jpeg_huff_check(b.desc.data(), 1, b.byte_total, (int64_t)b.sets.size(), b.coef_total, opt);
  CHECK(why == nullptr, "%s@%zu: descriptor refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  why = jpeg_huff_rst_check(b.desc.data(), 1, b.rst_items.data(), (int64_t)b.rst_items.size());
  CHECK(why == nullptr, "%s@%zu: items refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  CHECK(d.gpu == 1 || d.gpu == 4, "%s@%zu: gpu flag %d\n", what, at, d.gpu);
  if (d.gpu != 1 && d.gpu != 4) return -1;
  CHECK(d.gpu == 4 || b.rst_items.empty(), "%s@%zu: items of a one-lane entry\n", what, at);
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the lanes may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  std::unique_ptr<JpegHuffSet> set(new JpegHuffSet(b.sets[(size_t)d.set_idx]));
  int verdict = kJpegHuffOk;
  if (d.gpu == 4) {
    *intervals = true;
    const size_t ni = b.rst_items.size();
    g_items += descending ? 0 : (long)ni;
    for (size_t q = 0; q < ni; ++q) {
      const JpegRstItem& it = b.rst_items[descending ? ni - 1 - q : q];
      const int st = jpeg_huff_decode_interval(d, span.get(), *set, out.get(), it.byte_begin, it.mcu_first, it.index);
      CHECK(st == kJpegHuffOk || st == kJpegHuffCorrupt, "%s@%zu: interval status %d\n", what, at, st);
      if (st > verdict) verdict = st;
    }
  } else {
    verdict = jpeg_huff_decode_scan(d, span.get(), *set, out.get());
  }
  coefs->assign(out.get(), out.get() + d.total_coefs);
  return verdict;
}

static void compare(const uint8_t* data, size_t n, const char* what, size_t at, bool must_ok) {
  // the input in its own exactly sized heap copy
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), data, n);
  const uint8_t* ptr = n ? in.get() : nullptr;
  JpegHeader h;
  std::memset(&h, 0, sizeof(h));
  const int ps = jpeg_parse_header(ptr, n, &h);
  std::vector<int16_t> want(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(ptr, n, &h, want.data(), want.size());
  std::vector<int16_t> up, down;
  bool iv_up = false, iv_down = false;
  const int su = run_rst(ptr, n, false, what, at, &up, &iv_up);
  const int sd = run_rst(ptr, n, true, what, at, &down, &iv_down);
  CHECK(su == hs, "%s@%zu: ascending items %d, host decoder %d\n", what, at, su, hs);
  CHECK(sd == hs, "%s@%zu: descending items %d, host decoder %d\n", what, at, sd, hs);
  CHECK(iv_up == iv_down, "%s@%zu: the two plans differ\n", what, at);
  CHECK(up == down, "%s@%zu: coefficients depend on the item order\n", what, at);
  if (su == JPEG_OK && hs == JPEG_OK) CHECK(up == want, "%s@%zu: coefficients differ\n", what, at);
  if (must_ok) {
    CHECK(hs == JPEG_OK, "%s: host decoder status %d, expected ok\n", what, hs);
    CHECK(iv_up, "%s: a restart-interval file did not take the interval path\n", what);
  }
  if (ps != JPEG_OK) ++g_refused;
  else if (iv_up) ++(hs == JPEG_OK ? g_rst_ok : g_rst_corrupt);
  else ++(hs == JPEG_OK ? g_lane_ok : g_lane_corrupt);
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
  CHECK(argc > 1, "usage: jpeg_huff_rst_checks FILE.jpg...\n");
  long calls = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> d;
    if (!read_file(argv[a], &d) || d.empty()) {
      CHECK(false, "cannot read %s\n", argv[a]);
      continue;
    }
    compare(d.data(), d.size(), argv[a], d.size(), true);
    ++calls;
    for (size_t n = 0; n < d.size(); ++n) {
      compare(d.data(), n, argv[a], n, false);
      ++calls;
    }
    for (size_t p = 0; p < d.size(); p += 7) {
      const uint8_t vals[3] = {0xFF, 0x00, (uint8_t)(d[p] ^ 0x55)};
      for (int v = 0; v < 3; ++v) {
        ++calls;
        std::vector<uint8_t> m(d);
        m[p] = vals[v];
        compare(m.data(), m.size(), "mutant", p, false);
      }
    }
  }
  std::printf("interval path: both ok %ld, both refused %ld (%ld items)\n", g_rst_ok, g_rst_corrupt, g_items);
  std::printf("one-lane path: both ok %ld, both refused %ld; refused by the parse %ld\n", g_lane_ok, g_lane_corrupt,
              g_refused);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
