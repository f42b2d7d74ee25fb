// Host-side differential checks of the sub-stream Huffman decode
// (csrc/jpeg_huff_par.h) and its packer layout (runtime/jpeg_huff_pack.cpp with
// par_sub_bits) against the host decoder (runtime/jpeg_entropy.cpp), built
// together under host AddressSanitizer + UndefinedBehaviorSanitizer.
//
// The workgroup of jpeg_entropy_par_kernel is emulated sequentially: T virtual
// threads run each phase of jpeg_huff_par.h one after the other, a phase boundary
// standing for the kernel's barrier (the entries are double-buffered, so the order
// of the virtual threads inside a round does not matter).  For every file named on
// the command line it decodes
//   * the file itself (must be JPEG_OK),
//   * every prefix of it,
//   * the file with every 7th byte replaced in turn by FF, by 00 and by its value
//     XOR 55,
// at sub-stream sizes of 32 bits and kJpegParSubBits, each with T = 1, 3 and 64,
// with the image's word span, coefficient span and state span each in an exactly
// sized heap allocation.  Each run must give jpeg_decode's verdict and, where both
// are OK, identical coefficients.  At 32 bits the rounds are bounded by the number
// of sub-streams alone; at kJpegParSubBits by kJpegParMaxRounds as in the kernel,
// and the number of inputs that reached it is printed (the test wants none).
// --shard I N (first) keeps only the decode calls whose running number is I modulo N,
// so that the test can spread one pass over several processes; the counts add up.
// Build + run: tests/test_jpeg_huff_par_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../jpeg_huff_par.h"
#include "../runtime/jpeg_entropy.h"
#include "../runtime/jpeg_huff_pack.h"

using namespace idunno;

static int g_fail = 0;
static long g_both_ok = 0, g_both_corrupt = 0, g_refused = 0, g_mut_ok = 0, g_mut_corrupt = 0, g_unsynced = 0;
static uint32_t g_rounds_small = 0, g_rounds_kernel = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

// packer + the emulated workgroup on data[0, n); returns the verdict (the parse's when it refuses)
static int run_par(const uint8_t* ptr, size_t n, uint32_t S, uint32_t T, uint32_t rmax, const char* what, size_t at,
                   std::vector<int16_t>* coefs, uint32_t* rounds) {
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, S);
  coefs->clear();
  *rounds = 0;
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0, "%s@%zu: refused entry marked for the device\n", what, at);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  const JpegParDesc& p = b.par[0];
  const char* why = jpeg_huff_par_check(b.desc.data(), b.par.data(), 1, b.byte_total, (int64_t)b.sets.size(),
                                        b.coef_total, b.scratch_total, S);
  CHECK(why == nullptr, "%s@%zu: descriptor refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  CHECK(d.gpu == 2, "%s@%zu: a file without restart markers was not laid out for the sub-stream form\n", what, at);
  if (d.gpu != 2) return -1;
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the lanes may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  std::unique_ptr<JpegHuffSet> set(new JpegHuffSet(b.sets[(size_t)d.set_idx]));
  const uint32_t nsub = jpeg_par_nsub(p.bit_len, S);
  CHECK((int64_t)kJpegParStateWords * nsub == b.scratch_total, "%s@%zu: scratch span\n", what, at);
  std::unique_ptr<uint32_t[]> st(new uint32_t[(size_t)kJpegParStateWords * nsub]);
  const JpegParCtx x{&d, &p, span.get(), set.get(), st.get(), out.get(), S, nsub};

  for (uint32_t t = 0; t < T; ++t) jpeg_par_init(x, t, T);
  const uint32_t R = nsub < rmax ? nsub : rmax;
  int cur = 0;
  bool converged = false;
  for (uint32_t r = 0; r < R && !converged; ++r) {
    bool any = false;
    for (uint32_t t = 0; t < T; ++t) any = jpeg_par_round(x, cur, t, T) || any;
    ++*rounds;
    if (!any) converged = true;
    else cur ^= 1;
  }
  if (!converged) return kJpegHuffUnsynced;
  std::vector<uint32_t> part(4 * (size_t)T);
  for (uint32_t t = 0; t < T; ++t) jpeg_par_partial(x, t, T, &part[4 * (size_t)t]);
  uint32_t base[4] = {0u, 0u, 0u, 0u};
  for (uint32_t t = 0; t < T; ++t) {
    jpeg_par_scan(x, t, T, base);
    for (int q = 0; q < 4; ++q) base[q] += part[4 * (size_t)t + q];
  }
  int verdict = base[0] < p.total_blocks ? kJpegHuffCorrupt : kJpegHuffOk;   // the stream ends before the scan does
  for (uint32_t t = 0; t < T; ++t)
    if (jpeg_par_write(x, cur, t, T) != kJpegHuffOk) verdict = kJpegHuffCorrupt;
  coefs->assign(out.get(), out.get() + d.total_coefs);
  return verdict;
}

static void compare(const uint8_t* data, size_t n, const char* what, size_t at, bool must_ok, bool mutant) {
  // the input in its own exactly sized heap copy
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), data, n);
  const uint8_t* ptr = n ? in.get() : nullptr;
  JpegHeader h;
  std::memset(&h, 0, sizeof(h));
  const int ps = jpeg_parse_header(ptr, n, &h);
  std::vector<int16_t> want(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(ptr, n, &h, want.data(), want.size());
  int st = hs;
  static const uint32_t kT[3] = {1u, 3u, 64u};
  for (int form = 0; form < 2; ++form) {
    const uint32_t S = form ? kJpegParSubBits : 32u;
    for (int ti = 0; ti < 3; ++ti) {
      std::vector<int16_t> got;
      uint32_t rounds = 0;
      st = run_par(ptr, n, S, kT[ti], form ? kJpegParMaxRounds : 0xFFFFFFFFu, what, at, &got, &rounds);
      uint32_t& most = form ? g_rounds_kernel : g_rounds_small;
      if (rounds > most) most = rounds;
      if (st == kJpegHuffUnsynced) {
        ++g_unsynced;
        CHECK(false, "%s@%zu: S %u T %u: not converged after %u rounds\n", what, at, S, kT[ti], rounds);
        continue;
      }
      CHECK(st == hs, "%s@%zu: S %u T %u: sub-streams %d, host decoder %d\n", what, at, S, kT[ti], st, hs);
      if (st == JPEG_OK && hs == JPEG_OK) CHECK(got == want, "%s@%zu: S %u T %u: coefficients differ\n", what, at, S, kT[ti]);
    }
  }
  if (must_ok) CHECK(hs == JPEG_OK, "%s: host decoder status %d, expected ok\n", what, hs);
  if (hs == JPEG_OK) {
    ++g_both_ok;
    g_mut_ok += mutant;
  } else if (hs == JPEG_CORRUPT && ps == JPEG_OK) {
    ++g_both_corrupt;                       // refused by the entropy stage itself
    g_mut_corrupt += mutant;
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
  CHECK(argc > 1, "usage: jpeg_huff_par_checks FILE.jpg...\n");
  long calls = 0, seen = 0, shard = 0, nshard = 1;
  int first = 1;
  if (argc > 3 && std::strcmp(argv[1], "--shard") == 0) {
    shard = std::atol(argv[2]);
    nshard = std::atol(argv[3]);
    first = 4;
    CHECK(nshard >= 1 && shard >= 0 && shard < nshard, "bad --shard\n");
    if (nshard < 1) nshard = 1;
  }
  auto mine = [&]() { return seen++ % nshard == shard; };
  for (int a = first; a < argc; ++a) {
    std::vector<uint8_t> d;
    if (!read_file(argv[a], &d) || d.empty()) {
      CHECK(false, "cannot read %s\n", argv[a]);
      continue;
    }
    if (mine()) {
      compare(d.data(), d.size(), argv[a], d.size(), true, false);
      ++calls;
    }
    for (size_t n = 0; n < d.size(); ++n) {
      if (!mine()) continue;
      compare(d.data(), n, argv[a], n, false, false);
      ++calls;
    }
    for (size_t p = 0; p < d.size(); p += 7) {
      const uint8_t vals[3] = {0xFF, 0x00, (uint8_t)(d[p] ^ 0x55)};
      for (int v = 0; v < 3; ++v) {
        if (!mine()) continue;
        ++calls;
        std::vector<uint8_t> m(d);
        m[p] = vals[v];
        compare(m.data(), m.size(), "mutant", p, false, true);
      }
    }
  }
  std::printf("both ok %ld, both corrupt in the scan %ld, refused by the parse %ld\n", g_both_ok, g_both_corrupt,
              g_refused);
  std::printf("mutants: both ok %ld, both corrupt in the scan %ld\n", g_mut_ok, g_mut_corrupt);
  std::printf("largest round count at 32 bits %u, at %u bits %u (cap %u, reached by %ld)\n", g_rounds_small,
              kJpegParSubBits, g_rounds_kernel, kJpegParMaxRounds, g_unsynced);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
