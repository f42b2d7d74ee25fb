// Host-side differential checks of the 4:4:0 (luma 1x2, mode 3) and 4:1:1 (luma 4x1,
// mode 4) layouts that native_sampling admits: the host decoder
// (runtime/jpeg_entropy.cpp) against every form the device entropy stage has, each
// driven on the host from the packer's layout (runtime/jpeg_huff_pack.cpp) as its
// kernel drives it, built together under host AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
// For every file named on the command line (baseline, with restart markers, or
// progressive) it takes
//   * the file itself (must be JPEG_OK with mode 3 or 4, and JPEG_UNSUPPORTED_SAMPLING
//     without the flag),
//   * every prefix of it,
//   * the file with every 7th byte replaced in turn by FF, by 00 and by its value
//     XOR 55,
// decodes it with jpeg_decode (native_progressive and native_sampling on) and plans it
// three times with the same two flags:
//   * one-lane form: a gpu == 1 entry through jpeg_huff_decode_scan (jpeg_huff_core.h),
//   * sub-stream form (par_sub_bits = 32 and kJpegParSubBits): a gpu == 2 entry through
//     the phases of jpeg_huff_par.h with T virtual threads, as
//     csrc/tests/jpeg_huff_par_checks.cpp emulates the workgroup,
//   * interval form (restart_intervals): a gpu == 4 entry through
//     jpeg_huff_decode_interval (jpeg_huff_rst.h), one item after the other, the verdict
//     their maximum.
// In every form a gpu == 3 entry (progressive) goes through jpeg_prog_decode_image
// (jpeg_huff_prog.h) and whatever else the plan leaves to the one-lane kernel through
// jpeg_huff_decode_scan.  Word span, coefficient span, state span, scans and tables lie
// in exactly sized heap allocations.  Every run must give jpeg_decode's verdict and,
// where both accept, identical coefficients; every descriptor must pass the checks that
// run before a launch with native_sampling and, where its layout is a new one, be refused
// without.
// Build + run: tests/test_jpeg_sampling_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../jpeg_huff_core.h"
#include "../jpeg_huff_par.h"
#include "../jpeg_huff_prog.h"
#include "../jpeg_huff_rst.h"
#include "../runtime/jpeg_entropy.h"
#include "../runtime/jpeg_huff_pack.h"

using namespace idunno;

static int g_fail = 0;
static long g_both_ok = 0, g_both_corrupt = 0, g_refused = 0, g_unsynced = 0;
static long g_forms[5] = {0, 0, 0, 0, 0};       // runs by gpu flag
static uint32_t g_rounds = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

enum Form { kLane = 0, kParSmall = 1, kParKernel = 2, kIntervals = 3 };
static const char* const kFormName[4] = {"one-lane", "sub-streams of 32 bits", "sub-streams of the kernel's size", "intervals"};

static bool new_layout(const JpegHuffDesc& d) {
  return d.ncomp == 3 && d.h[1] == 1 && d.v[1] == 1 && d.h[2] == 1 && d.v[2] == 1 &&
         ((d.h[0] == 1 && d.v[0] == 2) || (d.h[0] == 4 && d.v[0] == 1));
}

// the emulated workgroup of jpeg_entropy_par_kernel on a gpu == 2 entry
static int run_substreams(const JpegHuffBatch& b, const uint32_t* span, const JpegHuffSet& set, int16_t* out, uint32_t S,
                          uint32_t T, uint32_t rmax) {
  const JpegHuffDesc& d = b.desc[0];
  const JpegParDesc& p = b.par[0];
  const uint32_t nsub = jpeg_par_nsub(p.bit_len, S);
  if ((int64_t)kJpegParStateWords * nsub != b.scratch_total) return -1;
  std::unique_ptr<uint32_t[]> st(new uint32_t[(size_t)kJpegParStateWords * nsub]);
  const JpegParCtx x{&d, &p, span, &set, st.get(), out, S, nsub};
  for (uint32_t t = 0; t < T; ++t) jpeg_par_init(x, t, T);
  const uint32_t R = nsub < rmax ? nsub : rmax;
  int cur = 0;
  bool converged = false;
  uint32_t rounds = 0;
  for (uint32_t r = 0; r < R && !converged; ++r) {
    bool any = false;
    for (uint32_t t = 0; t < T; ++t) any = jpeg_par_round(x, cur, t, T) || any;
    ++rounds;
    if (!any) converged = true;
    else cur ^= 1;
  }
  if (S == kJpegParSubBits && rounds > g_rounds) g_rounds = rounds;
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
  return verdict;
}

// progressive files always, the colour spaces never: without and with the new samplings
static JpegOptions progressive_only() { JpegOptions o; o.native_progressive = true; return o; }
static JpegOptions with_sampling() { JpegOptions o = progressive_only(); o.native_sampling = true; return o; }
static const JpegOptions kPlain = progressive_only(), kSampling = with_sampling();

// packer + the form's core(s) on data[0, n); returns the verdict (the parse's when it refuses)
static int run_form(const uint8_t* ptr, size_t n, Form form, const char* what, size_t at, std::vector<int16_t>* coefs) {
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  const uint32_t S = form == kParSmall ? 32u : (form == kParKernel ? kJpegParSubBits : 0u);
  const bool intervals = form == kIntervals;
  JpegOptions opt = kSampling, plain_opt = kPlain;
  opt.restart_intervals = plain_opt.restart_intervals = intervals;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, S, opt);
  coefs->clear();
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0 && b.rst_items.empty(), "%s@%zu %s: refused entry marked for the device\n", what, at,
          kFormName[form]);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  const int64_t nsets = (int64_t)b.sets.size();
  const char* why = S ? jpeg_huff_par_check(b.desc.data(), b.par.data(), 1, b.byte_total, nsets, b.coef_total,
                                            b.scratch_total, S, opt)
                      : jpeg_huff_check(b.desc.data(), 1, b.byte_total, nsets, b.coef_total, opt);
  if (why == nullptr)
    why = jpeg_huff_prog_check(b.desc.data(), 1, b.scans.data(), (int64_t)b.scans.size(), (int64_t)b.tabs.size());
  if (why == nullptr) why = jpeg_huff_rst_check(b.desc.data(), 1, b.rst_items.data(), (int64_t)b.rst_items.size());
  CHECK(why == nullptr, "%s@%zu %s: descriptor refused: %s\n", what, at, kFormName[form], why ? why : "");
  if (why != nullptr) return -1;
  // the same descriptor without native_sampling: refused exactly where the layout is one of the new two
  const char* plain = S ? jpeg_huff_par_check(b.desc.data(), b.par.data(), 1, b.byte_total, nsets, b.coef_total,
                                              b.scratch_total, S, plain_opt)
                        : jpeg_huff_check(b.desc.data(), 1, b.byte_total, nsets, b.coef_total, plain_opt);
  CHECK((plain != nullptr) == new_layout(d), "%s@%zu %s: check without native_sampling: %s\n", what, at, kFormName[form],
        plain ? plain : "accepted");
  const bool flag_ok = d.gpu == 1 || d.gpu == 3 || (d.gpu == 2 && S) || (d.gpu == 4 && intervals);
  CHECK(flag_ok, "%s@%zu %s: gpu flag %d\n", what, at, kFormName[form], d.gpu);
  if (!flag_ok) return -1;
  CHECK((d.gpu == 3) == (hdr.progressive == 1), "%s@%zu %s: gpu flag %d of a %s file\n", what, at, kFormName[form], d.gpu,
        hdr.progressive ? "progressive" : "baseline");
  CHECK(!(S && d.gpu == 1 && hdr.restart_interval == 0), "%s@%zu %s: not laid out for the sub-stream form\n", what, at,
        kFormName[form]);
  ++g_forms[d.gpu];
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the cores may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  int verdict = kJpegHuffOk;
  if (d.gpu == 3) {
    std::unique_ptr<JpegProgScan[]> scans(new JpegProgScan[b.scans.size()]);
    std::memcpy(scans.get(), b.scans.data(), b.scans.size() * sizeof(JpegProgScan));
    std::unique_ptr<JpegHuffTab[]> tabs(new JpegHuffTab[b.tabs.size()]);
    std::memcpy(tabs.get(), b.tabs.data(), b.tabs.size() * sizeof(JpegHuffTab));
    verdict = jpeg_prog_decode_image(d, scans.get(), (long long)b.scans.size(), span.get(), tabs.get(),
                                     (int32_t)b.tabs.size(), out.get());
  } else {
    std::unique_ptr<JpegHuffSet> set(new JpegHuffSet(b.sets[(size_t)d.set_idx]));
    if (d.gpu == 2) {
      verdict = run_substreams(b, span.get(), *set, out.get(), S, form == kParSmall ? 3u : 64u,
                               form == kParSmall ? 0xFFFFFFFFu : kJpegParMaxRounds);
      CHECK(verdict != -1, "%s@%zu %s: scratch span\n", what, at, kFormName[form]);
    } else if (d.gpu == 4) {
      for (const JpegRstItem& it : b.rst_items) {
        const int st = jpeg_huff_decode_interval(d, span.get(), *set, out.get(), it.byte_begin, it.mcu_first, it.index);
        CHECK(st == kJpegHuffOk || st == kJpegHuffCorrupt, "%s@%zu: interval status %d\n", what, at, st);
        if (st > verdict) verdict = st;
      }
    } else {
      verdict = jpeg_huff_decode_scan(d, span.get(), *set, out.get());
    }
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
  const int ps = jpeg_parse_header(ptr, n, &h, kSampling);
  std::vector<int16_t> want(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(ptr, n, &h, want.data(), want.size(), kSampling);
  for (int f = 0; f < 4; ++f) {
    std::vector<int16_t> got;
    const int st = run_form(ptr, n, (Form)f, what, at, &got);
    if (st == kJpegHuffUnsynced) {
      ++g_unsynced;
      CHECK(false, "%s@%zu %s: not converged\n", what, at, kFormName[f]);
      continue;
    }
    CHECK(st == hs, "%s@%zu %s: %d, host decoder %d\n", what, at, kFormName[f], st, hs);
    if (st == JPEG_OK && hs == JPEG_OK) CHECK(got == want, "%s@%zu %s: coefficients differ\n", what, at, kFormName[f]);
  }
  if (must_ok) {
    CHECK(hs == JPEG_OK, "%s: host decoder status %d, expected ok\n", what, hs);
    CHECK(h.ncomp == 3 && (h.mode == 3 || h.mode == 4), "%s: mode %d, expected 3 or 4\n", what, h.mode);
    CHECK((h.mode == 3 && h.comp[0].h == 1 && h.comp[0].v == 2) || (h.mode == 4 && h.comp[0].h == 4 && h.comp[0].v == 1),
          "%s: mode %d with luma %dx%d\n", what, h.mode, h.comp[0].h, h.comp[0].v);
    JpegHeader h2;
    CHECK(jpeg_parse_header(ptr, n, &h2, kPlain) == JPEG_UNSUPPORTED_SAMPLING, "%s: taken without native_sampling\n", what);
    std::vector<int16_t> none(want.size(), 0);
    CHECK(jpeg_decode(ptr, n, &h2, none.data(), none.size(), kPlain) == JPEG_UNSUPPORTED_SAMPLING,
          "%s: decoded without native_sampling\n", what);
  }
  if (hs == JPEG_OK) ++g_both_ok;
  else if (hs == JPEG_CORRUPT && ps == JPEG_OK) ++g_both_corrupt;       // refused by the entropy stage itself
  else ++g_refused;
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
  CHECK(argc > 1, "usage: jpeg_sampling_checks FILE.jpg...\n");
  long calls = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> d;
    if (!read_file(argv[a], &d) || d.empty()) {
      CHECK(false, "cannot read %s\n", argv[a]);
      continue;
    }
    compare(d.data(), d.size(), argv[a], d.size(), true);
    ++calls;
    for (size_t n = 0; n < d.size(); ++n, ++calls) compare(d.data(), n, argv[a], n, false);
    for (size_t p = 0; p < d.size(); p += 7) {
      const uint8_t vals[3] = {0xFF, 0x00, (uint8_t)(d[p] ^ 0x55)};
      for (int v = 0; v < 3; ++v, ++calls) {
        std::vector<uint8_t> m(d);
        m[p] = vals[v];
        compare(m.data(), m.size(), "mutant", p, false);
      }
    }
  }
  std::printf("both ok %ld, both corrupt in the scan %ld, refused by the parse %ld\n", g_both_ok, g_both_corrupt, g_refused);
  std::printf("runs by layout: one-lane %ld, sub-stream %ld, progressive %ld, interval %ld\n", g_forms[1], g_forms[2],
              g_forms[3], g_forms[4]);
  std::printf("largest round count at %u bits %u (cap %u, reached by %ld)\n", kJpegParSubBits, g_rounds, kJpegParMaxRounds,
              g_unsynced);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
