// Index math of the float-input kernels (kernels/float_input.hip) and of the
// packed-row stem geometry their outputs share with preprocess_pack3* and
// conv2d_pack3*.  __host__ __device__ so csrc/tests/float_input_checks.cpp
// (host ASan + UBSan) runs the exact functions the kernel inlines.
//
// A workgroup stages a band of image rows in LDS as fp32 words, one LDS row per
// image row holding the row's 3W "live" values interleaved: word g = channel
// g % 3 of pixel g / 3.  Every LDS access is a 4-byte access whose lanes are a
// fixed number of words apart:
//     stage, channels-last source   lane = 16 bytes of the row      stride 4 (fp32) / 8 (fp16)
//     stage, NCHW source            lane = 16 bytes of one plane    stride 12 / 24
//     nhwc4 fp32 / fp16 output      lane = 1 / 2 pixels             stride 3 / 6
//     packed rows, fp32 / fp16      lane = one 16-byte chunk        stride 4 / 8
// fi_phys pads five words after every sixteen: with it the 32 lanes the LDS
// serves per clock fall on 32 distinct banks (of 64) for each of these strides
// at every base word (asserted by the host checks).
#pragma once
#include <hip/hip_runtime.h>

namespace idunno {

constexpr int kFiThreads = 256;          // 4 waves
constexpr int kFiBandRows = 8;           // image rows per workgroup (fewer for very wide images)
constexpr int kFiLdsBytes = 48 * 1024;   // LDS budget of a workgroup

// Packed-row geometry of an RGB stem (conv_f32 mode 2 / conv_glds pack3, preprocess_pack3*,
// float_to_pack3*): nc row copies (the distinct 16-byte phases of 3*stride*ox for E = 16 /
// elem_bytes elements per chunk), wp elements each, cpk 16-byte chunks per kernel row.
__host__ __device__ inline void pack3_geometry_of(int W, int KW, int stride, int pad, int elem_bytes, int& nc,
                                                  int& wp, int& cpk) {
  const int E = 16 / elem_bytes;
  int g = 1;                                   // gcd(3 * stride, E), E a power of two
  while (g < E && (3 * stride) % (2 * g) == 0) g *= 2;
  nc = E / g;
  wp = (3 * (W + 2 * pad) + E - 1 + E - 1) / E * E;
  cpk = (3 * KW + E - 1) / E;
}

// Element i of copy c of a packed row is R[i + c * g], g = E / nc, where R[f] = channel f % 3 of
// pixel f / 3 - pad and zero outside the image.  The live word (0 .. 3W - 1) behind element i, or
// -1 where the packed row holds padding.
__host__ __device__ __forceinline__ int pack3_live_word(int i, int c, int g, int pad, int W) {
  const int w = i + c * g - 3 * pad;
  return (w >= 0 && w < 3 * W) ? w : -1;
}

// LDS word of live word g within its row
__host__ __device__ __forceinline__ int fi_phys(int g) { return g + (g >> 4) * 5; }
// LDS words per staged row of an image W pixels wide
__host__ __device__ __forceinline__ int fi_pitch(int W) { return fi_phys(3 * W - 1) + 1; }
// Rows per band: kFiBandRows, fewer where a band would not fit the LDS budget; 0 = a row does not fit
__host__ __device__ __forceinline__ int fi_band_rows(int W) {
  const long rows = kFiLdsBytes / (4L * fi_pitch(W));
  return rows > kFiBandRows ? kFiBandRows : (int)rows;
}
// Band b of an image H rows tall: rows [y0, y0 + nr)
__host__ __device__ __forceinline__ void fi_band(int b, int rows, int H, int& y0, int& nr) {
  y0 = b * rows;
  nr = H - y0 < rows ? H - y0 : rows;
}

// A source segment (a channels-last row or one plane's row) is n contiguous elements of
// elem_bytes each, starting at byte address `addr`, which may be anywhere (views).  Its items:
// item 0 = the `head` elements before the first 16-byte boundary, then whole 16-byte vectors,
// the last item = what is left.  Every item of VE = 16 / elem_bytes elements is a 16-byte
// aligned vector load; shorter ones are loaded element by element.
__host__ __device__ __forceinline__ int fi_head(unsigned long long addr, int elem_bytes, int n) {
  const int h = (int)((16 - (addr & 15)) & 15) / elem_bytes;
  return h < n ? h : n;
}
__host__ __device__ __forceinline__ int fi_items(int n, int head, int VE) { return 1 + (n - head + VE - 1) / VE; }
// elements [lo, hi) of item t
__host__ __device__ __forceinline__ void fi_item(int t, int n, int head, int VE, int& lo, int& hi) {
  lo = t == 0 ? 0 : head + (t - 1) * VE;
  hi = t == 0 ? head : lo + VE;
  if (hi > n) hi = n;
}
// live word of element e of a segment: channels-last (ch < 0) or plane ch of an NCHW image
__host__ __device__ __forceinline__ int fi_seg_word(int e, int ch) { return ch < 0 ? e : 3 * e + ch; }

// nhwc4 fp16: a pixel is 8 bytes, so an item is the pixel pair that shares a 16-byte slot of the
// output.  `par` = parity of the row's first pixel in the whole output; item k covers pixels
// [2k - par, 2k - par + 2) clipped to the row (a clipped item is one 8-byte store).
__host__ __device__ __forceinline__ int fi_pair_items(int W, int par) { return (W + par + 1) / 2; }
__host__ __device__ __forceinline__ void fi_pair(int k, int par, int W, int& x0, int& x1) {
  x0 = 2 * k - par;
  x1 = x0 + 2;
  if (x0 < 0) x0 = 0;
  if (x1 > W) x1 = W;
}

}  // namespace idunno
