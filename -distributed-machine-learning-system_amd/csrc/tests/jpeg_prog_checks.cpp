// Host-side differential checks of the progressive JPEG path: the marker walk
// (runtime/jpeg_entropy.cpp), the packer's gpu == 3 layout
// (runtime/jpeg_huff_pack.cpp) and the shared core (csrc/jpeg_huff_prog.h), built
// together under host AddressSanitizer + UndefinedBehaviorSanitizer.
//
// Arguments: pairs PROGRESSIVE.jpg BASELINE.jpg of the same pixels and settings.
// For every pair
//   (a) the host path (jpeg_decode, native_progressive) on the progressive file
//       must give the coefficients jpeg_decode gives for the baseline twin,
//   (b) the packed path -- jpeg_huff_plan / jpeg_huff_copy_bytes, both checks, the
//       image's byte span, its scan range, the table buffer and its coefficient
//       span each in an exactly sized heap allocation, jpeg_prog_decode_image
//       driven as the kernel drives it -- must give the host path's status and,
//       where both accept, identical coefficients: for the file, for every prefix
//       of it, and with every 7th byte replaced by FF, by 00 and by its value
//       XOR 55,
//   (c) the sanitizers must stay silent and no call may run more loop trips than
//       scans x blocks x (64 + 1) x 64, far above what the core's own bounds allow.
// Build + run: tests/test_jpeg_prog_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../jpeg_huff_prog.h"
#include "../runtime/jpeg_entropy.h"
#include "../runtime/jpeg_huff_pack.h"

using namespace idunno;

static int g_fail = 0;
static long g_both_ok = 0, g_both_refused = 0;
static long long g_max_trips = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

static JpegOptions progressive() { JpegOptions o; o.native_progressive = true; return o; }
static const JpegOptions kProgressive = progressive();

// packer + core on data[0, n) from its own exactly sized heap copy; returns the verdict
static int run_packed(const uint8_t* data, size_t n, const char* what, size_t at, std::vector<int16_t>* coefs) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), data, n);
  const uint8_t* ptr = n ? in.get() : nullptr;
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, 0, kProgressive);
  coefs->clear();
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0, "%s@%zu: refused entry marked for the device\n", what, at);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  CHECK(d.gpu == 3 && hdr.progressive == 1, "%s@%zu: accepted entry is not a progressive one\n", what, at);
  if (d.gpu != 3) return -1;
  const char* why = jpeg_huff_check(b.desc.data(), 1, b.byte_total, (int64_t)b.sets.size(), b.coef_total, kProgressive);
  if (why == nullptr)
    why = jpeg_huff_prog_check(b.desc.data(), 1, b.scans.data(), (int64_t)b.scans.size(), (int64_t)b.tabs.size());
  CHECK(why == nullptr, "%s@%zu: descriptor refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  CHECK(jpeg_huff_check(b.desc.data(), 1, b.byte_total, (int64_t)b.sets.size(), b.coef_total) != nullptr,
        "%s@%zu: the baseline check took a progressive entry\n", what, at);
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the core may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<JpegProgScan[]> scans(new JpegProgScan[b.scans.size()]);
  std::memcpy(scans.get(), b.scans.data(), b.scans.size() * sizeof(JpegProgScan));
  std::unique_ptr<JpegHuffTab[]> tabs(new JpegHuffTab[b.tabs.size()]);
  std::memcpy(tabs.get(), b.tabs.data(), b.tabs.size() * sizeof(JpegHuffTab));
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  long long trips = 0;
  const int st = jpeg_prog_decode_image(d, scans.get(), (long long)b.scans.size(), span.get(), tabs.get(),
                                        (int32_t)b.tabs.size(), out.get(), &trips);
  const long long bound = (long long)d.nscans * (d.total_coefs / 64) * 65 * 64;
  CHECK(trips <= bound, "%s@%zu: %lld loop trips, bound %lld\n", what, at, trips, bound);
  if (trips > g_max_trips) g_max_trips = trips;
  coefs->assign(out.get(), out.get() + d.total_coefs);
  return st;
}

// host path against packed path; want != nullptr: the twin's coefficients, which both must give
static void compare(const uint8_t* data, size_t n, const char* what, size_t at, const std::vector<int16_t>* want) {
  std::vector<int16_t> got;
  const int st = run_packed(data, n, what, at, &got);
  JpegHeader h;
  std::memset(&h, 0, sizeof(h));
  const int ps = jpeg_parse_header(n ? data : nullptr, n, &h, kProgressive);
  std::vector<int16_t> host(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(n ? data : nullptr, n, &h, host.data(), host.size(), kProgressive);
  CHECK(st == hs, "%s@%zu: packed path %d, host path %d\n", what, at, st, hs);
  if (want != nullptr) {
    CHECK(hs == JPEG_OK && st == JPEG_OK, "%s: status %d / %d, expected ok\n", what, hs, st);
    CHECK(h.progressive == 1 && h.nscans >= 2, "%s: not a progressive file\n", what);
    CHECK(host == *want, "%s: host path differs from the baseline twin\n", what);
    // without the option the file is refused as before
    CHECK(jpeg_parse_header(data, n, &h) == JPEG_UNSUPPORTED_PROGRESSIVE, "%s: default parse took it\n", what);
  }
  if (st == JPEG_OK && hs == JPEG_OK) {
    ++g_both_ok;
    CHECK(got == host, "%s@%zu: coefficients differ\n", what, at);
  } else if (st == hs) {
    ++g_both_refused;
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
  CHECK(argc > 2 && argc % 2 == 1, "usage: jpeg_prog_checks PROGRESSIVE.jpg BASELINE.jpg ...\n");
  long calls = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    std::vector<uint8_t> d, twin;
    if (!read_file(argv[a], &d) || d.empty() || !read_file(argv[a + 1], &twin) || twin.empty()) {
      CHECK(false, "cannot read %s / %s\n", argv[a], argv[a + 1]);
      continue;
    }
    JpegHeader th;
    std::memset(&th, 0, sizeof(th));
    CHECK(jpeg_parse_header(twin.data(), twin.size(), &th) == JPEG_OK, "%s: twin refused\n", argv[a + 1]);
    std::vector<int16_t> want(th.total_coefs, 0);
    CHECK(jpeg_decode(twin.data(), twin.size(), &th, want.data(), want.size()) == JPEG_OK, "%s: twin refused\n",
          argv[a + 1]);
    compare(d.data(), d.size(), argv[a], d.size(), &want);
    ++calls;
    for (size_t n = 0; n < d.size(); ++n, ++calls) compare(d.data(), n, argv[a], n, nullptr);
    for (size_t p = 0; p < d.size(); p += 7) {
      const uint8_t repl[3] = {0xFF, 0x00, (uint8_t)(d[p] ^ 0x55)};
      for (int r = 0; r < 3; ++r, ++calls) {
        std::vector<uint8_t> m(d);
        m[p] = repl[r];
        compare(m.data(), m.size(), "mutant", p, nullptr);
      }
    }
  }
  std::printf("most loop trips in one call %lld\n", g_max_trips);
  std::printf("%ld decode calls, both ok %ld, both refused %ld, %d failure(s)\n", calls, g_both_ok, g_both_refused,
              g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
