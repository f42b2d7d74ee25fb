// Index math of the grouped 3x3 conv (kernels/conv3x3_grouped.hip), shared with
// the host-side checker (csrc/tests/grouped_checks.cpp, host ASan + UBSan) and the
// binding's shape checks.  __host__ __device__ so the checker drives the exact
// functions the kernel inlines.
//
// A conv with `groups` groups of Cg = C / groups channels is channel-block-local:
// with CB = max(16, Cg), output channels [CB j, CB j + CB) read input channels of
// the same range only.  Per block the weights are a small dense [CB outputs, 9 taps,
// CB inputs] matrix (zeros outside an output's own group when Cg < 16) whose K
// axis runs k = tap * CB + ci, cut into MFMA K-steps of 32.
#pragma once
#include <hip/hip_runtime.h>

namespace idunno {
namespace grouped {

constexpr int kSlab = 64;   // channels a workgroup owns (four 16-output MFMA fragments, one per wave)
constexpr int kTW = 16;     // output columns of a pixel group (the MFMA's N)
constexpr int kPad = 8;     // halfs of padding after a staged pixel's channels (LDS bank spread)

__host__ __device__ constexpr bool cg_ok(int cg) {
  return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64;
}
// channel block of a group size
__host__ __device__ constexpr int block_of(int cg) { return cg < 16 ? 16 : cg; }
// K-steps (of 32) over a block's 9 * CB weights; CB 16: 4.5 -> 5, the last half step is zero
__host__ __device__ constexpr int ksteps(int cb) { return (9 * cb + 31) / 32; }

// K slot kk of a channel block -> (tap, input channel within the block); tap 9 is
// the zero half step of CB 16 (never read from memory, neither weights nor pixels)
struct KSlot {
  int tap, ci;
};
__host__ __device__ __forceinline__ KSlot kslot(int cb, int kk) { return {kk / cb, kk % cb}; }

// Packing map: input channel (within its group) that slot `ci` of output channel
// `co`'s block row holds, or -1 where the slot belongs to another group (zero).
__host__ __device__ __forceinline__ int slot_group_ci(int cg, int co, int ci) {
  const int cb = block_of(cg);
  return ci / cg == (co % cb) / cg ? ci % cg : -1;
}

// First slab channel of the block that the slab's 16-output fragment `frag` (= wave) lies in
__host__ __device__ constexpr int frag_block_base(int cb, int frag) { return (16 * frag) / cb * cb; }

// ---- tile geometry --------------------------------------------------------------
// A workgroup computes tile_rows(stride) x 16 output pixels from a staged input
// patch of in_rows x in_cols pixels whose first pixel is input (oy0 * stride - 1,
// ox0 * stride - 1); pixels outside the image are staged as zeros (the padding).
__host__ __device__ constexpr int tile_rows(int stride) { return stride == 1 ? 8 : 2; }
__host__ __device__ constexpr int in_rows(int stride) { return (tile_rows(stride) - 1) * stride + 3; }
__host__ __device__ constexpr int in_cols(int stride) { return (kTW - 1) * stride + 3; }

struct InPixel {
  int iy, ix;
  bool inside;
};
// staged pixel (r, c) of the tile at output (oy0, ox0)
__host__ __device__ __forceinline__ InPixel in_pixel(int oy0, int ox0, int stride, int r, int c, int H, int W) {
  const int iy = oy0 * stride - 1 + r, ix = ox0 * stride - 1 + c;
  return {iy, ix, iy >= 0 && iy < H && ix >= 0 && ix < W};
}
// staged pixel index that output (row g, column col) of the tile reads at `tap` (< 9)
__host__ __device__ __forceinline__ int lds_pixel(int g, int col, int tap, int stride) {
  return (g * stride + tap / 3) * in_cols(stride) + col * stride + tap % 3;
}
// halfs from one staged pixel to the next: its channels (64, or 128 split) + kPad
__host__ __device__ constexpr int lds_pitch(bool split) { return (split ? 2 : 1) * kSlab + kPad; }
// half offset of slab channel c (8-aligned) within a staged / global pixel; split: the hi half, lo at +32
__host__ __device__ __forceinline__ int chan_off(bool split, int c) {
  return split ? ((c >> 5) << 6) + (c & 31) : c;
}

__host__ __device__ constexpr int out_size(int n, int stride) { return (n + 2 - 3) / stride + 1; }

}  // namespace grouped
}  // namespace idunno
