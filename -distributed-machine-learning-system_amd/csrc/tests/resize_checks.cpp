// Host-side checks of the uint8 resize + crop's host math (csrc/resize_math.h), built with
// host AddressSanitizer + UndefinedBehaviorSanitizer like grouped_checks.cpp: the exact
// functions the binding and resize_u8.hip use, on tables in heap buffers ASan watches.
// Per geometry (the tested ones, a 1 x N strip, an upscale, and two whose supports force the
// chunked form):
//   * every band's row range (band_rows) covers each of its rows' taps, stays inside the
//     image and fits the strip unless the plan is chunked (then the band is one row);
//     every column's taps lie inside the staged columns [xlo, xlo + xn) of the image;
//   * the fixed-point weights of every output sum to 1 << PRECISION_BITS within Pillow's
//     own rounding (half a unit per tap);
//   * the workgroup's LDS (tables, raw rows, strip) is under the budget and its parts do
//     not overlap;
//   * raw_slot: for every head 0..15 the slots of a staged row write each of the row's
//     bytes exactly once, inside raw_pitch, and whole slots are 16-byte aligned on both sides.
// Build + run: tests/test_resize_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../resize_math.h"
#include "../tile_math.h"

using namespace idunno::resize;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

static void check_axis(const char* what, int Hi, int Wi, const int* b, const int* k, int crop, int ksize, int in) {
  for (int o = 0; o < crop; ++o) {
    const int lo = b[2 * o], n = b[2 * o + 1];
    CHECK(lo >= 0 && n >= 1 && n <= ksize && lo + n <= in, "%dx%d %s %d: taps [%d, +%d) of %d\n", Hi, Wi, what, o, lo,
          n, in);
    long sum = 0;
    for (int t = 0; t < ksize; ++t) {
      const int w = k[o * ksize + t];
      CHECK(w >= 0 && (t < n || w == 0), "%dx%d %s %d: weight %d at tap %d\n", Hi, Wi, what, o, w, t);
      sum += w;
    }
    CHECK(std::labs(sum - (1L << kPrecisionBits)) <= (n + 1) / 2, "%dx%d %s %d: weights sum to %ld\n", Hi, Wi, what,
          o, sum);
    if (o) CHECK(lo >= b[2 * o - 2] && lo + n >= b[2 * o - 2] + b[2 * o - 1], "%dx%d %s %d: taps move back\n", Hi,
                 Wi, what, o);
  }
}

static void check_geometry(int Hi, int Wi, int resize, int crop, int want_chunked) {
  int Hr, Wr, top, left;
  idunno::resize_crop_geometry(Hi, Wi, resize, crop, Hr, Wr, top, left);
  const int ksh = ksize_of(Wi, Wr), ksv = ksize_of(Hi, Hr);
  std::vector<int> tab((size_t)table_ints(crop, ksh, ksv));
  std::vector<double> w((size_t)(ksh > ksv ? ksh : ksv));
  const Plan p = make_plan(Hi, Wi, Hr, Wr, top, left, crop, tab.data(), w.data());
  const int *bh = tab.data(), *kh = bh + 2 * crop, *bv = bh + p.off_bv, *kv = bh + p.off_kv;
  CHECK(p.tab_ints == (int)tab.size() && p.ksh == ksh && p.ksv == ksv, "%dx%d: table layout\n", Hi, Wi);
  check_axis("column", Hi, Wi, bh, kh, crop, ksh, Wi);
  check_axis("row", Hi, Wi, bv, kv, crop, ksv, Hi);
  CHECK(p.chunked == want_chunked, "%dx%d -> %d/%d: chunked %d\n", Hi, Wi, resize, crop, p.chunked);
  // columns: inside what a workgroup stages
  CHECK(p.xlo >= 0 && p.xn >= 1 && p.xlo + p.xn <= Wi, "%dx%d: staged columns [%d, +%d)\n", Hi, Wi, p.xlo, p.xn);
  for (int x = 0; x < crop; ++x)
    CHECK(bh[2 * x] >= p.xlo && bh[2 * x] + bh[2 * x + 1] <= p.xlo + p.xn, "%dx%d column %d outside the stage\n", Hi,
          Wi, x);
  // bands
  CHECK(p.band >= 1 && p.band <= kMaxBand && p.nbands == (crop + p.band - 1) / p.band, "%dx%d: band %d x %d\n", Hi,
        Wi, p.band, p.nbands);
  CHECK(!p.chunked || (p.band == 1 && (3 * crop + 15) / 16 <= kThreads), "%dx%d: chunked band %d\n", Hi, Wi, p.band);
  for (int r0 = 0; r0 < crop; r0 += p.band) {
    const int r1 = r0 + p.band < crop ? r0 + p.band : crop;
    int y0, y1;
    band_rows(bv, r0, r1, y0, y1);
    CHECK(y0 >= 0 && y0 < y1 && y1 <= Hi, "%dx%d band %d: rows [%d, %d)\n", Hi, Wi, r0, y0, y1);
    CHECK(p.chunked || y1 - y0 <= p.strip_rows, "%dx%d band %d: %d rows, strip %d\n", Hi, Wi, r0, y1 - y0,
          p.strip_rows);
    for (int r = r0; r < r1; ++r)
      CHECK(bv[2 * r] >= y0 && bv[2 * r] + bv[2 * r + 1] <= y1, "%dx%d row %d outside its band's rows\n", Hi, Wi, r);
  }
  // LDS
  const int tab_bytes = 4 * (crop * (2 + ksh) + p.band * (2 + ksv));
  CHECK(p.lds_bytes <= kLdsBudget && p.strip_rows >= 1 && p.raw_rows >= 1, "%dx%d: %d LDS bytes\n", Hi, Wi,
        p.lds_bytes);
  CHECK(p.lds_raw % 16 == 0 && p.lds_strip % 16 == 0 && p.raw_pitch % 16 == 0 && p.strip_pitch % 16 == 0 &&
            (p.strip_pitch / 16) % 2 == 1 && p.strip_pitch >= align16(3 * crop),
        "%dx%d: LDS alignment\n", Hi, Wi);
  CHECK(p.lds_raw >= (p.tab_lds ? tab_bytes : 0) && p.lds_strip >= p.lds_raw + p.raw_rows * p.raw_pitch &&
            p.lds_bytes >= p.lds_strip + p.strip_rows * p.strip_pitch,
        "%dx%d: LDS parts overlap\n", Hi, Wi);
  CHECK(!p.tab_lds || tab_bytes <= kTabBudget, "%dx%d: %d table bytes in LDS\n", Hi, Wi, tab_bytes);
  // staging of a row of 3 xn bytes at every alignment
  const int nbytes = 3 * p.xn;
  for (int head = 0; head < 16; ++head) {
    std::vector<int> hit((size_t)p.raw_pitch, 0);
    for (int v = 0; v < p.raw_pitch / 16; ++v) {
      const RawSlot s = raw_slot(head, v, nbytes);
      CHECK(!s.whole || (s.lo + head) % 16 == 0, "slot %d head %d: unaligned whole slot\n", v, head);
      for (int j = 0; j < 16; ++j)
        if (s.whole || (s.lo + j >= 0 && s.lo + j < nbytes)) {
          CHECK(s.lo + j >= 0 && s.lo + j < nbytes, "slot %d head %d reads byte %d of %d\n", v, head, s.lo + j, nbytes);
          hit[(size_t)(16 * v + j)]++;
        }
    }
    for (int o = 0; o < p.raw_pitch; ++o)
      CHECK(hit[(size_t)o] == (o >= head && o < head + nbytes), "%dx%d head %d: staged byte %d written %d times\n", Hi,
            Wi, head, o, hit[(size_t)o]);
  }
}

int main() {
  check_geometry(375, 500, 256, 224, 0);
  check_geometry(500, 375, 256, 224, 0);
  check_geometry(224, 224, 256, 224, 0);     // upscale, support 1
  check_geometry(256, 256, 256, 256, 0);     // identity
  check_geometry(225, 300, 256, 224, 0);
  check_geometry(30, 40, 32, 29, 0);
  check_geometry(17, 1031, 16, 16, 0);
  check_geometry(1031, 17, 16, 16, 0);
  check_geometry(1, 50, 8, 8, 0);            // a 1 x N strip
  check_geometry(50, 1, 8, 8, 0);
  check_geometry(7, 9, 256, 256, 0);         // a large upscale
  check_geometry(4000, 4100, 32, 32, 0);     // tables too large for LDS
  check_geometry(7680, 7680, 256, 256, 1);   // a row's support does not fit the strip
  check_geometry(16384, 16384, 1, 1, 1);
  check_geometry(16384, 16384, 256, 256, 1);
  std::printf("%d failure(s)\n", g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
