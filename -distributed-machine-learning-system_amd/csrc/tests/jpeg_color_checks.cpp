// Host-side differential checks of what native_colorspace admits: four-component files
// (CMYK, YCCK; every component 1x1) and RGB-coded three-component files.  The host decoder
// (runtime/jpeg_entropy.cpp) against the one-lane core (jpeg_huff_core.h) and the
// progressive scan core (jpeg_huff_prog.h), each driven on the host from the packer's
// layout (runtime/jpeg_huff_pack.cpp) as its kernel drives it, built together under host
// AddressSanitizer + UndefinedBehaviorSanitizer.
//
// For every file named on the command line (baseline, with restart markers, or
// progressive) it takes
//   * the file itself (must be JPEG_OK with the colour space its name says: cmyk*, ycck*,
//     rgb*; a four-component file must be JPEG_UNSUPPORTED_COMPONENTS without the flag and
//     a three-component one must parse to colorspace 0 without it),
//   * every prefix of it,
//   * the file with every 7th byte replaced in turn by FF, by 00 and by its value XOR 55,
// decodes it with jpeg_decode (native_progressive and native_colorspace on), plans it with
// the same two flags in the one-lane layout and runs the entry through
// jpeg_huff_decode_scan (gpu == 1) or jpeg_prog_decode_image (gpu == 3).  Word span,
// coefficient span, scans and tables lie in exactly sized heap allocations.  The run must
// give jpeg_decode's verdict and, where both accept, identical coefficients; the
// descriptor must pass the checks that run before a launch with native_colorspace and,
// where it has four components, be refused without.
// It also plans every input in the sub-stream layout, with restart_intervals and with
// both: a four-component entry must never get gpu == 2 or gpu == 4, and those plans must
// pass their checks too.
// Build + run: tests/test_jpeg_color_checks.py.  Exit status = number of failures.
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
static long g_both_ok = 0, g_both_corrupt = 0, g_refused = 0;
static long g_forms[5] = {0, 0, 0, 0, 0};       // core runs by gpu flag
static long g_four = 0, g_four_layouts = 0;     // four-component inputs accepted; their plans in the other layouts
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

// progressive files always, the new samplings never: without and with the colour spaces
static JpegOptions progressive_only() { JpegOptions o; o.native_progressive = true; return o; }
static JpegOptions with_colorspace() { JpegOptions o = progressive_only(); o.native_colorspace = true; return o; }
static const JpegOptions kPlain = progressive_only(), kColor = with_colorspace();

static const char* all_checks(const JpegHuffBatch& b, uint32_t S, const JpegOptions& opt) {
  const int64_t nsets = (int64_t)b.sets.size();
  const char* why = S ? jpeg_huff_par_check(b.desc.data(), b.par.data(), 1, b.byte_total, nsets, b.coef_total,
                                            b.scratch_total, S, opt)
                      : jpeg_huff_check(b.desc.data(), 1, b.byte_total, nsets, b.coef_total, opt);
  if (why == nullptr)
    why = jpeg_huff_prog_check(b.desc.data(), 1, b.scans.data(), (int64_t)b.scans.size(), (int64_t)b.tabs.size());
  if (why == nullptr) why = jpeg_huff_rst_check(b.desc.data(), 1, b.rst_items.data(), (int64_t)b.rst_items.size());
  return why;
}

// the packer's other layouts: no four-component entry on the sub-stream or the interval kernel
static void other_layouts(const uint8_t* ptr, size_t n, const char* what, size_t at) {
  for (int f = 1; f < 4; ++f) {
    const uint32_t S = (f & 1) ? kJpegParSubBits : 0u;
    JpegHeader hdr;
    int status = -1;
    JpegHuffBatch b;
    JpegOptions opt = kColor;
    opt.restart_intervals = (f & 2) != 0;
    jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, S, opt);
    if (status != JPEG_OK) continue;
    const JpegHuffDesc& d = b.desc[0];
    const char* why = all_checks(b, S, opt);
    CHECK(why == nullptr, "%s@%zu layout %d: descriptor refused: %s\n", what, at, f, why ? why : "");
    if (hdr.ncomp != 4) continue;
    ++g_four_layouts;
    CHECK(d.ncomp == 4 && (d.gpu == 1 || d.gpu == 3), "%s@%zu layout %d: four components with gpu flag %d\n", what, at, f,
          d.gpu);
    CHECK(b.rst_items.empty() && b.scratch_total == 0, "%s@%zu layout %d: four components with items or scratch\n", what,
          at, f);
  }
}

// packer + core in the one-lane layout on data[0, n); returns the verdict (the parse's when it refuses)
static int run_core(const uint8_t* ptr, size_t n, const char* what, size_t at, std::vector<int16_t>* coefs) {
  JpegHeader hdr;
  int status = -1;
  JpegHuffBatch b;
  jpeg_huff_plan(1, &ptr, &n, &hdr, &status, &b, 0u, kColor);
  coefs->clear();
  if (status != JPEG_OK) {
    CHECK(b.desc[0].gpu == 0 && b.rst_items.empty(), "%s@%zu: refused entry marked for the device\n", what, at);
    return status;
  }
  const JpegHuffDesc& d = b.desc[0];
  const char* why = all_checks(b, 0u, kColor);
  CHECK(why == nullptr, "%s@%zu: descriptor refused: %s\n", what, at, why ? why : "");
  if (why != nullptr) return -1;
  // the same descriptor without native_colorspace: refused exactly where it has four components
  const char* plain = all_checks(b, 0u, kPlain);
  CHECK((plain != nullptr) == (d.ncomp == 4), "%s@%zu: check without native_colorspace: %s\n", what, at,
        plain ? plain : "accepted");
  CHECK(d.ncomp == hdr.ncomp, "%s@%zu: %d components in the descriptor, %d in the header\n", what, at, d.ncomp, hdr.ncomp);
  CHECK(d.gpu == (hdr.progressive ? 3 : 1), "%s@%zu: gpu flag %d of a %s file\n", what, at, d.gpu,
        hdr.progressive ? "progressive" : "baseline");
  if (d.gpu != 1 && d.gpu != 3) return -1;
  ++g_forms[d.gpu];
  std::vector<uint8_t> all((size_t)b.byte_total);
  jpeg_huff_copy_bytes(b, &ptr, &n, all.data());
  // exact sizes: what the cores may touch of this image and not one byte more
  std::unique_ptr<uint32_t[]> span(new uint32_t[d.byte_span / 4]);
  if (d.byte_span) std::memcpy(span.get(), all.data() + d.byte_off, d.byte_span);
  std::unique_ptr<int16_t[]> out(new int16_t[d.total_coefs]);
  std::memset(out.get(), 0, (size_t)d.total_coefs * sizeof(int16_t));
  int verdict;
  if (d.gpu == 3) {
    std::unique_ptr<JpegProgScan[]> scans(new JpegProgScan[b.scans.size()]);
    std::memcpy(scans.get(), b.scans.data(), b.scans.size() * sizeof(JpegProgScan));
    std::unique_ptr<JpegHuffTab[]> tabs(new JpegHuffTab[b.tabs.size()]);
    std::memcpy(tabs.get(), b.tabs.data(), b.tabs.size() * sizeof(JpegHuffTab));
    verdict = jpeg_prog_decode_image(d, scans.get(), (long long)b.scans.size(), span.get(), tabs.get(),
                                     (int32_t)b.tabs.size(), out.get());
  } else {
    std::unique_ptr<JpegHuffSet> set(new JpegHuffSet(b.sets[(size_t)d.set_idx]));
    verdict = jpeg_huff_decode_scan(d, span.get(), *set, out.get());
  }
  coefs->assign(out.get(), out.get() + d.total_coefs);
  return verdict;
}

// expect: the colour space the intact file must have (1 RGB, 2 CMYK, 3 YCCK), 0: a prefix or mutant
static void compare(const uint8_t* data, size_t n, const char* what, size_t at, int expect) {
  // the input in its own exactly sized heap copy
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), data, n);
  const uint8_t* ptr = n ? in.get() : nullptr;
  JpegHeader h;
  std::memset(&h, 0, sizeof(h));
  const int ps = jpeg_parse_header(ptr, n, &h, kColor);
  std::vector<int16_t> want(ps == JPEG_OK ? h.total_coefs : 0, 0);
  const int hs = jpeg_decode(ptr, n, &h, want.data(), want.size(), kColor);
  CHECK(hs != JPEG_OK || (h.ncomp == 4 ? (h.colorspace == 2 || h.colorspace == 3) : h.ncomp == 3 ? h.colorspace <= 1
                                                                                                  : h.colorspace == 0),
        "%s@%zu: colour space %d of %d components\n", what, at, h.colorspace, h.ncomp);
  std::vector<int16_t> got;
  const int st = run_core(ptr, n, what, at, &got);
  CHECK(st == hs, "%s@%zu: core %d, host decoder %d\n", what, at, st, hs);
  if (st == JPEG_OK && hs == JPEG_OK) CHECK(got == want, "%s@%zu: coefficients differ\n", what, at);
  other_layouts(ptr, n, what, at);
  if (hs == JPEG_OK && h.ncomp == 4) ++g_four;
  if (expect) {
    CHECK(hs == JPEG_OK, "%s: host decoder status %d, expected ok\n", what, hs);
    CHECK(h.colorspace == expect && h.ncomp == (expect == 1 ? 3 : 4) && h.mode >= 0 && h.mode <= 2,
          "%s: colour space %d, %d components, expected %d\n", what, h.colorspace, h.ncomp, expect);
    for (int c = 0; c < h.ncomp && expect != 1; ++c)
      CHECK(h.at(c).h == 1 && h.at(c).v == 1 && h.at(c).bw == h.mcux && h.at(c).bh == h.mcuy, "%s: component %d not 1x1\n",
            what, c);
    JpegHeader h2;
    std::vector<int16_t> none(want.size(), 0);
    const int s2 = jpeg_parse_header(ptr, n, &h2, kPlain);
    if (expect == 1) {
      CHECK(s2 == JPEG_OK && h2.colorspace == 0, "%s: colour space %d without native_colorspace\n", what, h2.colorspace);
      CHECK(jpeg_decode(ptr, n, &h2, none.data(), none.size(), kPlain) == JPEG_OK && none == want,
            "%s: other coefficients without native_colorspace\n", what);
    } else {
      CHECK(s2 == JPEG_UNSUPPORTED_COMPONENTS, "%s: taken without native_colorspace\n", what);
      CHECK(jpeg_decode(ptr, n, &h2, none.data(), none.size(), kPlain) == JPEG_UNSUPPORTED_COMPONENTS,
            "%s: decoded without native_colorspace\n", what);
    }
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

// the colour space a file's name promises: cmyk* 2, ycck* 3, rgb* 1
static int expected(const char* path) {
  const char* base = std::strrchr(path, '/');
  base = base ? base + 1 : path;
  if (std::strncmp(base, "cmyk", 4) == 0) return 2;
  if (std::strncmp(base, "ycck", 4) == 0) return 3;
  if (std::strncmp(base, "rgb", 3) == 0) return 1;
  return -1;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: jpeg_color_checks FILE.jpg...\n");
  long calls = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> d;
    const int expect = expected(argv[a]);
    if (!read_file(argv[a], &d) || d.empty() || expect < 0) {
      CHECK(false, "cannot read %s, or its name says no colour space\n", argv[a]);
      continue;
    }
    compare(d.data(), d.size(), argv[a], d.size(), expect);
    ++calls;
    for (size_t n = 0; n < d.size(); ++n, ++calls) compare(d.data(), n, argv[a], n, 0);
    for (size_t p = 0; p < d.size(); p += 7) {
      const uint8_t vals[3] = {0xFF, 0x00, (uint8_t)(d[p] ^ 0x55)};
      for (int v = 0; v < 3; ++v, ++calls) {
        std::vector<uint8_t> m(d);
        m[p] = vals[v];
        compare(m.data(), m.size(), "mutant", p, 0);
      }
    }
  }
  std::printf("both ok %ld, both corrupt in the scan %ld, refused by the parse %ld\n", g_both_ok, g_both_corrupt, g_refused);
  std::printf("runs by layout: one-lane %ld, progressive %ld\n", g_forms[1], g_forms[3]);
  std::printf("four-component inputs decoded %ld, planned in the other layouts %ld\n", g_four, g_four_layouts);
  std::printf("%ld decode calls, %d failure(s)\n", calls, g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
