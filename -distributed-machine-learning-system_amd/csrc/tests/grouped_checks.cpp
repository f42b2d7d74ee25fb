// Host-side checks of the grouped 3x3 conv's index math (csrc/grouped_math.h), built
// with host AddressSanitizer + UndefinedBehaviorSanitizer like host_checks.cpp: the
// exact __host__ __device__ functions conv3x3_grouped.hip inlines, driven the way
// the kernel drives them.
//   * channel map: for every Cg in {4, 8, 16, 32, 64}, every C up to 2048 and every
//     output channel, the K-steps of the channel's wave read every (tap, input channel)
//     of the channel's group exactly once, every other slot they read is a zero slot
//     of the packing map and lies in the channel's own block, and 8-half operand
//     reads never straddle a tap, a block or a split hi/lo run;
//   * geometry: for H, W = 1 .. 20 and both strides, a 1-channel integer conv computed
//     through the staged patch (in_pixel -> patch, lds_pixel -> taps) equals the direct
//     conv, the staging reads no pixel outside the image (ASan watches the buffers) and
//     no tile row or column of a whole MFMA fragment reads outside the patch.
// There is no swizzle to check: staged pixels are padded by kPad halfs instead.
// Build + run: tests/test_grouped_checks.py.  Exit status = number of failures.
#include <cstdio>
#include <vector>

#include "../grouped_math.h"

using namespace idunno::grouped;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (g_fail++ < 20) std::printf(__VA_ARGS__);     \
    }                                                  \
  } while (0)

static void check_channel_map() {
  const int cgs[] = {4, 8, 16, 32, 64};
  for (int cg : cgs) {
    CHECK(cg_ok(cg), "cg_ok(%d) false\n", cg);
    const int cb = block_of(cg), ks = ksteps(cb);
    CHECK(cb >= 16 && cb % cg == 0 && kSlab % cb == 0, "block_of(%d) = %d\n", cg, cb);
    CHECK(32 * ks >= 9 * cb && 32 * (ks - 1) < 9 * cb, "ksteps(%d) = %d\n", cb, ks);
    for (int C = 32; C <= 2048; C += 32) {
      if (C % cg || C / cg < 2) continue;
      for (int stride = 1; stride <= 2; ++stride) {      // the channel map does not depend on it
        for (int co = 0; co < C; ++co) {
          const int slab = co / kSlab, wave = (co % kSlab) / 16;
          const int nch = C - slab * kSlab < kSlab ? C - slab * kSlab : kSlab;
          CHECK(16 * wave < nch, "Cg %d C %d: channel %d on an idle wave\n", cg, C, co);
          const int bbase = frag_block_base(cb, wave);
          std::vector<int> seen(9 * cg, 0);
          for (int s = 0; s < ks; ++s)
            for (int kq = 0; kq < 4; ++kq) {
              const int kk = 32 * s + 8 * kq;
              const KSlot k = kslot(cb, kk);
              if (k.tap >= 9) {                          // the kernel reads neither weights nor pixels here
                CHECK(kk >= 9 * cb, "Cg %d: slot %d skipped inside the weights\n", cg, kk);
                continue;
              }
              CHECK(kk + 8 <= 9 * cb, "Cg %d: weight read at %d past the row\n", cg, kk);
              CHECK(k.ci % 8 == 0 && k.ci + 8 <= cb, "Cg %d: operand read at slot %d straddles a tap\n", cg, kk);
              const int c0 = bbase + k.ci;               // first slab channel of the 8 read
              CHECK(c0 + 8 <= nch, "Cg %d C %d co %d: reads slab channel %d of %d\n", cg, C, co, c0, nch);
              CHECK((c0 & 31) + 8 <= 32, "split run straddled at slab channel %d\n", c0);
              CHECK(chan_off(false, c0) == c0 && chan_off(true, c0) + 32 + 8 <= 2 * kSlab,
                    "chan_off(%d) outside the staged pixel\n", c0);
              for (int j = 0; j < 8; ++j) {
                const int cin = slab * kSlab + c0 + j;
                CHECK(cin / cb == co / cb, "Cg %d C %d: output %d reads channel %d of another block\n", cg, C, co, cin);
                const int gi = slot_group_ci(cg, co, k.ci + j);
                if (gi < 0) {
                  CHECK(cin / cg != co / cg, "Cg %d: zero slot inside output %d's group (channel %d)\n", cg, co, cin);
                } else {
                  CHECK(cin == co / cg * cg + gi, "Cg %d: output %d slot %d -> channel %d, want %d\n", cg, co,
                        k.ci + j, cin, co / cg * cg + gi);
                  seen[k.tap * cg + gi]++;
                }
              }
            }
          for (int i = 0; i < 9 * cg; ++i)
            CHECK(seen[i] == 1, "Cg %d C %d stride %d: output %d visits (tap %d, ci %d) %d times\n", cg, C, stride, co,
                  i / cg, i % cg, seen[i]);
        }
      }
    }
  }
  const int bad[] = {1, 2, 3, 12, 24, 128};
  for (int cg : bad) CHECK(!cg_ok(cg), "cg_ok(%d) true\n", cg);
}

static void check_geometry() {
  for (int stride = 1; stride <= 2; ++stride) {
    const int th = tile_rows(stride), ih = in_rows(stride), iw = in_cols(stride);
    CHECK(th % 2 == 0, "tile_rows(%d) = %d is odd (rows are stored in pairs)\n", stride, th);
    for (int H = 1; H <= 20; ++H)
      for (int W = 1; W <= 20; ++W) {
        const int Ho = out_size(H, stride), Wo = out_size(W, stride);
        CHECK(Ho == (H - 1) / stride + 1 && Wo == (W - 1) / stride + 1, "out_size(%d x %d, %d)\n", H, W, stride);
        std::vector<int> img(H * W);                     // exactly H * W: ASan sees any read outside
        for (int i = 0; i < H * W; ++i) img[i] = 1 + (i * 7919) % 101;
        const int wt[9] = {1, 2, 4, 8, 16, 32, 64, 128, 256};
        for (int oy0 = 0; oy0 < Ho; oy0 += th)
          for (int ox0 = 0; ox0 < Wo; ox0 += kTW) {
            std::vector<int> patch(ih * iw);
            for (int r = 0; r < ih; ++r)
              for (int c = 0; c < iw; ++c) {
                const InPixel p = in_pixel(oy0, ox0, stride, r, c, H, W);
                const bool in = p.iy >= 0 && p.iy < H && p.ix >= 0 && p.ix < W;
                CHECK(p.inside == in, "in_pixel inside flag wrong at (%d, %d)\n", p.iy, p.ix);
                patch[r * iw + c] = p.inside ? img[p.iy * W + p.ix] : 0;
              }
            for (int g = 0; g < th; ++g)
              for (int col = 0; col < kTW; ++col) {
                int got = 0;
                for (int tap = 0; tap < 9; ++tap) {
                  const int idx = lds_pixel(g, col, tap, stride);
                  CHECK(idx >= 0 && idx < ih * iw, "lds_pixel(%d, %d, %d, %d) = %d outside the patch\n", g, col, tap,
                        stride, idx);
                  if (idx >= 0 && idx < ih * iw) got += wt[tap] * patch[idx];
                }
                const int oy = oy0 + g, ox = ox0 + col;
                if (oy >= Ho || ox >= Wo) continue;
                int want = 0;
                for (int dy = 0; dy < 3; ++dy)
                  for (int dx = 0; dx < 3; ++dx) {
                    const int iy = oy * stride - 1 + dy, ix = ox * stride - 1 + dx;
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) want += wt[3 * dy + dx] * img[iy * W + ix];
                  }
                CHECK(got == want, "%d x %d stride %d: output (%d, %d) = %d through the patch, %d direct\n", H, W,
                      stride, oy, ox, got, want);
              }
          }
      }
  }
  CHECK(lds_pitch(false) % 8 == 0 && lds_pitch(true) % 8 == 0, "staged pixels must keep 16-byte alignment\n");
}

int main() {
  check_channel_map();
  check_geometry();
  std::printf("grouped_checks: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}
