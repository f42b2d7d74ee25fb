// Host-side checks of the float-input kernels' index math (csrc/float_input_math.h), built
// with host AddressSanitizer + UndefinedBehaviorSanitizer like resize_checks.cpp: the exact
// functions float_input.hip inlines, run in the kernel's own order on heap buffers of the
// exact size (a wrong index is an ASan report, not a silent pass).
//   * fi_phys: injective inside fi_pitch, and for every access stride of the kernel (3, 4,
//     6, 8, 12, 24 words between lanes) and every base word the 32 lanes of a half wave
//     fall on 32 distinct banks of 64;
//   * fi_head / fi_items / fi_item: for every misalignment, both element sizes and short
//     to long segments the items cover each element exactly once, and every full item is
//     a 16-byte aligned vector inside the segment;
//   * bands: fi_band covers each row once, ragged last band included, under the LDS budget;
//   * whole kernel, emulated per band: stage (NCHW planes or a channels-last row, through
//     the items) into an LDS image, then every form's destination row -- nhwc4 fp32, the
//     nhwc4 fp16 pixel pairs (16-byte slots, 8-byte clipped ends), packed rows for
//     7x7/2 pad 3, 11x11/4 pad 2 and 5x5/1 pad 2 at 4- and 2-byte elements (not the
//     8-copy 5x5/1 fp16 geometry, which the bindings refuse) -- against the
//     layouts' definitions; every destination element is written exactly once.
// Build + run: tests/test_float_input_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../float_input_math.h"

using namespace idunno;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

static void check_banks() {
  std::vector<char> seen(fi_pitch(1400), 0);
  for (int g = 0; g < 3 * 1400; ++g) {
    const int p = fi_phys(g);
    CHECK(p >= 0 && p < (int)seen.size() && !seen[p], "fi_phys(%d) = %d collides or leaves the pitch\n", g, p);
    if (p >= 0 && p < (int)seen.size()) seen[p] = 1;
  }
  const int strides[] = {3, 4, 6, 8, 12, 24};
  for (int s : strides)
    for (int base = 0; base < 2048; ++base) {
      unsigned long long banks = 0;
      for (int l = 0; l < 32; ++l) {
        const unsigned long long bit = 1ull << (fi_phys(base + s * l) & 63);
        CHECK(!(banks & bit), "stride %d base %d: lane %d shares a bank\n", s, base, l);
        banks |= bit;
      }
    }
}

static void check_items() {
  for (int eb = 2; eb <= 4; eb += 2) {
    const int VE = 16 / eb;
    for (int mis = 0; mis < 16; mis += eb)
      for (int n = 1; n < 80; ++n) {
        const unsigned long long addr = 4096 + mis;
        const int head = fi_head(addr, eb, n), items = fi_items(n, head, VE);
        std::vector<int> hit(n, 0);
        for (int t = 0; t < items; ++t) {
          int lo, hi;
          fi_item(t, n, head, VE, lo, hi);
          CHECK(lo >= 0 && hi <= n && lo <= hi, "eb %d mis %d n %d item %d: [%d, %d)\n", eb, mis, n, t, lo, hi);
          if (hi - lo == VE) CHECK((addr + (unsigned long long)lo * eb) % 16 == 0, "eb %d mis %d n %d item %d unaligned\n", eb, mis, n, t);
          for (int e = lo; e < hi; ++e) ++hit[e];
        }
        for (int e = 0; e < n; ++e) CHECK(hit[e] == 1, "eb %d mis %d n %d: element %d loaded %d times\n", eb, mis, n, e, hit[e]);
      }
  }
}

// value of channel ch of pixel (y, x): distinct and never 0
static float val(int y, int x, int ch) { return (float)(1 + ch + 3 * (x + 1000 * y)); }

// One image of H x W through the kernel's two phases, band by band.  `mis`: misalignment
// (elements) of the source rows; eb: source element bytes (only the item split depends on it).
static void check_image(int H, int W, bool cl, int mis, int eb) {
  const int VE = 16 / eb, rows = fi_band_rows(W), pitch = fi_pitch(W);
  CHECK(rows >= 1 && 4L * rows * pitch <= kFiLdsBytes, "W %d: %d rows of %d words over the LDS budget\n", W, rows, pitch);
  if (rows < 1) return;
  const int nbands = (H + rows - 1) / rows;
  std::vector<int> row_seen(H, 0);
  // destinations, exact size, with a write count per element
  std::vector<float> n4(4L * H * W);
  std::vector<int> n4_hit(n4.size(), 0), n4h_hit(n4.size(), 0);
  struct Geo { int kw, stride, pad; };
  const Geo geos[] = {{7, 2, 3}, {11, 4, 2}, {5, 1, 2}};
  for (int band = 0; band < nbands; ++band) {
    int y0, nr;
    fi_band(band, rows, H, y0, nr);
    CHECK(nr >= 1 && nr <= rows && y0 + nr <= H, "H %d band %d: rows [%d, +%d)\n", H, band, y0, nr);
    for (int r = 0; r < nr; ++r) ++row_seen[y0 + r];
    std::vector<float> lds((size_t)nr * pitch, -1.f);      // exactly the band: ragged bands stay inside
    // ---- stage ----
    const int n = cl ? 3 * W : W;
    for (int s = 0; s < (cl ? nr : 3 * nr); ++s) {
      const int r = cl ? s : s / 3, ch = cl ? -1 : s % 3;
      std::vector<float> seg(n);                             // the source segment
      for (int e = 0; e < n; ++e) seg[e] = cl ? val(y0 + r, e / 3, e % 3) : val(y0 + r, e, ch);
      const unsigned long long addr = 4096 + (unsigned long long)mis * eb;
      const int head = fi_head(addr, eb, n), items = fi_items(n, head, VE);
      for (int t = 0; t < items; ++t) {
        int lo, hi;
        fi_item(t, n, head, VE, lo, hi);
        for (int e = lo; e < hi; ++e) lds[(size_t)r * pitch + fi_phys(fi_seg_word(e, ch))] = seg[e];
      }
    }
    // ---- nhwc4 fp32: one pixel per lane ----
    for (int r = 0; r < nr; ++r)
      for (int x = 0; x < W; ++x) {
        const long o = ((long)(y0 + r) * W + x) * 4;
        for (int c = 0; c < 3; ++c) n4[o + c] = lds[(size_t)r * pitch + fi_phys(3 * x + c)];
        n4[o + 3] = 0.f;
        for (int c = 0; c < 4; ++c) ++n4_hit[o + c];
      }
    // ---- nhwc4 fp16: pixel pairs on 16-byte slots of the whole output ----
    for (int r = 0; r < nr; ++r) {
      const int p0 = (y0 + r) * W, par = p0 & 1;
      for (int k = 0; k < fi_pair_items(W, par); ++k) {
        int x0, x1;
        fi_pair(k, par, W, x0, x1);
        CHECK(x0 >= 0 && x1 <= W && x1 - x0 >= 1 && x1 - x0 <= 2, "W %d par %d pair %d: [%d, %d)\n", W, par, k, x0, x1);
        if (x1 - x0 == 2) CHECK(((p0 + x0) & 1) == 0, "W %d par %d pair %d: 16-byte store off its slot\n", W, par, k);
        for (int x = x0; x < x1; ++x)
          for (int c = 0; c < 4; ++c) ++n4h_hit[((long)p0 + x) * 4 + c];
      }
    }
    // ---- packed rows ----
    for (const Geo& g : geos)
      for (int ob = 2; ob <= 4; ob += 2) {
        int nc, wp, cpk;
        pack3_geometry_of(W, g.kw, g.stride, g.pad, ob, nc, wp, cpk);
        const int E = 16 / ob, G = E / nc;
        if (nc > 4) continue;                                // refused by the bindings (5x5/1 at 2-byte elements)
        CHECK(nc >= 1 && wp % E == 0, "W %d kw %d: nc %d wp %d\n", W, g.kw, nc, wp);
        std::vector<float> out((size_t)nr * nc * wp, -1.f);
        for (int rc = 0; rc < nr * nc; ++rc) {
          const int r = rc / nc, c = rc % nc;
          for (int j = 0; j < wp / E; ++j)
            for (int i = 0; i < E; ++i) {
              const int w = pack3_live_word(E * j + i, c, G, g.pad, W);
              CHECK(w >= -1 && w < 3 * W, "live word %d\n", w);
              out[((size_t)r * nc + c) * wp + E * j + i] = w >= 0 ? lds[(size_t)r * pitch + fi_phys(w)] : 0.f;
            }
        }
        // the layout's definition: element i of copy c = R[i + c*G], R[f] = pixel f/3 - pad, channel f%3
        for (int r = 0; r < nr; ++r)
          for (int c = 0; c < nc; ++c)
            for (int i = 0; i < wp; ++i) {
              const int f = i + c * G, x = f / 3 - g.pad;
              const float want = (x >= 0 && x < W) ? val(y0 + r, x, f % 3) : 0.f;
              CHECK(out[((size_t)r * nc + c) * wp + i] == want, "%dx%d kw %d eb %d row %d copy %d el %d: %g, want %g\n", H,
                    W, g.kw, ob, y0 + r, c, i, out[((size_t)r * nc + c) * wp + i], want);
            }
        // what the consumer reads for output pixel ox, kernel row: 3*KW elements from R[3*stride*ox]
        const int Wo = (W + 2 * g.pad - g.kw) / g.stride + 1;
        for (int ox = 0; ox < Wo; ++ox) {
          const int f = 3 * g.stride * ox, c = (f % E) / G, i0 = f - c * G;
          CHECK((f % E) % G == 0 && c < nc && i0 % E == 0 && i0 + cpk * E <= wp,
                "W %d kw %d eb %d ox %d: chunk run [%d, +%d) of copy %d\n", W, g.kw, ob, ox, i0, cpk * E, c);
        }
      }
  }
  for (int y = 0; y < H; ++y) CHECK(row_seen[y] == 1, "H %d: row %d in %d bands\n", H, y, row_seen[y]);
  for (size_t i = 0; i < n4.size(); ++i) {
    const int c = (int)(i % 4), x = (int)(i / 4 % W), y = (int)(i / 4 / W);
    CHECK(n4_hit[i] == 1 && n4h_hit[i] == 1, "%dx%d nhwc4 element %zu written %d / %d times\n", H, W, i, n4_hit[i], n4h_hit[i]);
    CHECK(n4[i] == (c < 3 ? val(y, x, c) : 0.f), "%dx%d nhwc4 (%d,%d,%d) = %g\n", H, W, y, x, c, n4[i]);
  }
}

int main() {
  check_banks();
  check_items();
  const int shapes[][2] = {{37, 45}, {224, 224}, {1, 1}, {9, 2}, {8, 64}, {17, 131}, {3, 1365}};
  for (const auto& s : shapes)
    for (int cl = 0; cl < 2; ++cl)
      for (int eb = 2; eb <= 4; eb += 2)
        for (int mis = 0; mis < 16 / eb; mis += (s[0] > 100 ? 3 : 1)) check_image(s[0], s[1], cl != 0, mis, eb);
  CHECK(fi_band_rows(3 * 1365) < kFiBandRows && fi_band_rows(1 << 20) == 0, "band rows of very wide images\n");
  std::printf("%d failure(s)\n", g_fail);
  return g_fail > 255 ? 255 : g_fail;
}
