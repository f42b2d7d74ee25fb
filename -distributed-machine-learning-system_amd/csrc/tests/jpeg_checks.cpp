// Host-side checks of the JPEG entropy decoder (csrc/runtime/jpeg_entropy.cpp),
// built together with it under host AddressSanitizer + UndefinedBehaviorSanitizer.
// For every file named on the command line it decodes
//   * the file itself (must be JPEG_OK),
//   * every prefix of it,
//   * the file with one byte replaced, at every 7th position, by a value from
//     a fixed LCG,
// each into an exactly sized heap buffer between guard words.  Every call must
// return a status of the enum and leave the guards intact; the sanitizers catch
// any access outside the input or output span.  Also: a short output buffer is
// refused, and the threaded batch entry agrees with the single calls.
// Build + run: tests/test_jpeg_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../runtime/jpeg_entropy.h"

using namespace idunno;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

constexpr size_t kGuard = 32;
constexpr int16_t kGuardWord = 0x5A5A;

// decode data[0, n) from its own exactly sized heap copy into a guarded buffer
static int decode_guarded(const uint8_t* data, size_t n, const char* what, size_t at, std::vector<int16_t>* keep) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);   // exact size: ASan sees a read past the span
  if (n) std::memcpy(in.get(), data, n);
  JpegHeader hdr;
  std::memset(&hdr, 0, sizeof(hdr));
  const int ps = jpeg_parse_header(n ? in.get() : nullptr, n, &hdr);
  CHECK(ps >= 0 && ps < JPEG_STATUS_COUNT, "%s@%zu: parse status %d\n", what, at, ps);
  const size_t total = ps == JPEG_OK ? hdr.total_coefs : 0;
  std::vector<int16_t> buf(total + 2 * kGuard, kGuardWord);
  JpegHeader h2;
  std::memset(&h2, 0, sizeof(h2));
  const int st = jpeg_decode(n ? in.get() : nullptr, n, &h2, buf.data() + kGuard, total);
  CHECK(st >= 0 && st < JPEG_STATUS_COUNT, "%s@%zu: status %d\n", what, at, st);
  if (ps != JPEG_OK) CHECK(st == ps, "%s@%zu: parse %d but decode %d\n", what, at, ps, st);
  for (size_t i = 0; i < kGuard; ++i)
    CHECK(buf[i] == kGuardWord && buf[kGuard + total + i] == kGuardWord, "%s@%zu: guard overwritten\n", what, at);
  if (keep != nullptr) keep->assign(buf.begin() + kGuard, buf.begin() + kGuard + total);
  return st;
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
  CHECK(argc > 1, "usage: jpeg_checks FILE.jpg...\n");
  std::vector<std::vector<uint8_t>> files;
  std::vector<std::vector<int16_t>> coefs;
  long calls = 0;
  uint32_t lcg = 12345u;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> d;
    if (!read_file(argv[a], &d) || d.empty()) {
      CHECK(false, "cannot read %s\n", argv[a]);
      continue;
    }
    std::vector<int16_t> c;
    const int st = decode_guarded(d.data(), d.size(), argv[a], d.size(), &c);
    CHECK(st == JPEG_OK, "%s: status %s, expected ok\n", argv[a], jpeg_status_name(st));
    ++calls;
    // a buffer one element short is refused, and untouched
    if (st == JPEG_OK && !c.empty()) {
      std::vector<int16_t> small(c.size() - 1 + kGuard, kGuardWord);
      JpegHeader h;
      const int s2 = jpeg_decode(d.data(), d.size(), &h, small.data(), c.size() - 1);
      CHECK(s2 == JPEG_BUFFER_TOO_SMALL, "%s: short buffer gave %d\n", argv[a], s2);
      for (int16_t w : small) CHECK(w == kGuardWord, "%s: short buffer written\n", argv[a]);
    }
    for (size_t n = 0; n < d.size(); ++n, ++calls) decode_guarded(d.data(), n, argv[a], n, nullptr);
    for (size_t p = 0; p < d.size(); p += 7, ++calls) {
      lcg = lcg * 1664525u + 1013904223u;
      std::vector<uint8_t> m(d);
      m[p] = (uint8_t)(lcg >> 24);
      decode_guarded(m.data(), m.size(), "mutant", p, nullptr);
    }
    files.push_back(std::move(d));
    coefs.push_back(std::move(c));
  }
  // the batch entry: 3 threads, one missing entry, results equal to the single calls
  const int n = (int)files.size() + 1;
  std::vector<const uint8_t*> ptr(n, nullptr);
  std::vector<size_t> len(n, 0), cap(n, 0);
  std::vector<std::vector<int16_t>> outs(n);
  std::vector<int16_t*> optr(n, nullptr);
  std::vector<JpegHeader> hdr(n);
  std::vector<int> status(n, -1);
  for (int i = 0; i + 1 < n; ++i) {
    ptr[i] = files[i].data();
    len[i] = files[i].size();
    outs[i].assign(coefs[i].size(), kGuardWord);
    optr[i] = outs[i].data();
    cap[i] = outs[i].size();
  }
  jpeg_decode_batch(n, ptr.data(), len.data(), hdr.data(), optr.data(), cap.data(), status.data(), 3);
  for (int i = 0; i + 1 < n; ++i)
    CHECK(status[i] == JPEG_OK && outs[i] == coefs[i], "batch entry %d differs (status %d)\n", i, status[i]);
  CHECK(status[n - 1] == JPEG_EMPTY, "missing batch entry gave %d\n", status[n - 1]);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
