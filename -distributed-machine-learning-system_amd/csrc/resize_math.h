// Host math of the uint8 resize + centre crop (kernels/resize_u8.hip), shared with the
// binding (bind_elementwise.cpp) and the host-side checker (csrc/tests/resize_checks.cpp,
// host ASan + UBSan).  __host__ __device__ and free of the standard library, so the
// checker drives the exact functions the binding and the kernel use.
//
// The filter is Pillow's Image.resize(..., BILINEAR) on 8-bit pixels (Resample.c):
// precompute_coeffs in double precision, normalize_coeffs_8bpc to fixed point with
// PRECISION_BITS = 32 - 8 - 2, a horizontal pass and a vertical pass that each start
// from 1 << (PRECISION_BITS - 1), shift and clip to 8 bits.  The centre crop is applied
// to the tables: only the crop's output columns and rows get coefficients.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace idunno {
namespace resize {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int kThreads = 256;
constexpr int kLdsBudget = 64 * 1024;   // per workgroup: two workgroups share a CU's LDS
constexpr int kTabBudget = 20 * 1024;   // coefficient tables up to this size are copied into LDS
constexpr int kMaxCrop = 256;
constexpr int kMaxDim = 16384;
constexpr int kMaxBand = 16;            // output rows of a workgroup, at most
constexpr int kRawRows = 8;             // input rows staged per step, at most

__host__ __device__ constexpr int align16(int n) { return (n + 15) & ~15; }

// taps per output of an axis resized in -> out: Pillow's ksize for the support-1 triangle
__host__ __device__ inline int ksize_of(int in, int out) {
  double fs = (double)in / out;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(fs) * 2 + 1;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for outputs [first, first + n) of an
// axis resized in -> out (box = the whole axis): bounds[2 o] = first tap, bounds[2 o + 1] =
// taps, kk[o * ksize + t] = fixed-point weight of tap t (zero past the taps).  `w` is
// scratch for ksize doubles.  Operation for operation as Pillow writes it, so the
// doubles round the same way.
__host__ __device__ inline void axis_coeffs(int in, int out, int first, int n, int ksize, int* bounds, int* kk,
                                            double* w) {
  double scale, filterscale;
  filterscale = scale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale, ss = 1.0 / filterscale;
  for (int o = 0; o < n; ++o) {
    const double center = 0.0 + (first + o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    for (int x = 0; x < ksize; ++x) {
      double k = 0.0;
      if (x < xmax) k = ww != 0.0 ? w[x] / ww : w[x];
      kk[o * ksize + x] = k < 0 ? (int)(-0.5 + k * (1 << kPrecisionBits)) : (int)(0.5 + k * (1 << kPrecisionBits));
    }
    bounds[2 * o] = xmin;
    bounds[2 * o + 1] = xmax;
  }
}

// Input rows [y0, y1) that output rows [r0, r1) of a bounds table touch.  First taps and
// tap ends both never decrease with the output index (a truncation and a clamp of an
// increasing centre), so the first and the last row give the range.
__host__ __device__ inline void band_rows(const int* bv, int r0, int r1, int& y0, int& y1) {
  y0 = bv[2 * r0];
  y1 = bv[2 * (r1 - 1)] + bv[2 * (r1 - 1) + 1];
}

// Staging of an input row: the row's first byte sits `head` (0..15, its address mod 16) bytes
// into 16-byte slot 0 of its staged copy, so slot v holds the row's bytes [lo, lo + 16) and
// global and LDS addresses are 16-byte aligned together.  A `whole` slot lies inside the
// row's nbytes and moves as one 16-byte load; the others move byte by byte, inside the row only.
struct RawSlot {
  int lo;
  bool whole;
};
__host__ __device__ inline RawSlot raw_slot(int head, int v, int nbytes) {
  const int lo = 16 * v - head;
  return {lo, lo >= 0 && lo + 16 <= nbytes};
}

// One geometry's launch plan.  The device table is int32 [bh | kh | bv | kv]: horizontal
// bounds [crop][2] and weights [crop][ksh], vertical bounds [crop][2] and weights [crop][ksv].
// A workgroup's LDS is [tables (tab_lds) | raw input rows | horizontally filtered strip].
struct Plan {
  int Hi, Wi, crop;
  int ksh, ksv;                  // taps per output, horizontal / vertical
  int xlo, xn;                   // input columns [xlo, xlo + xn) that the crop's columns touch
  int band, nbands;              // output rows per workgroup, workgroups per image
  int raw_rows, raw_pitch;       // input rows staged per step, bytes from one staged row to the next
  int strip_rows, strip_pitch;   // rows of the filtered strip, bytes from one to the next
  int chunked;                   // band == 1 and its input rows pass through the strip strip_rows at a time
  int tab_lds;                   // the tables are copied into LDS (else read from memory)
  int off_bv, off_kv, tab_ints;  // int offsets into the device table (bh at 0, kh at 2 crop)
  int lds_raw, lds_strip, lds_bytes;
};

__host__ __device__ inline int table_ints(int crop, int ksh, int ksv) { return crop * (2 + ksh) + crop * (2 + ksv); }

// The table (tab, table_ints ints; `w` scratch for max(ksh, ksv) doubles) and the plan of
// Hi x Wi -> resize_crop_geometry's (Hr, Wr, top, left) -> crop x crop.
__host__ __device__ inline Plan make_plan(int Hi, int Wi, int Hr, int Wr, int top, int left, int crop, int* tab,
                                          double* w) {
  Plan p{};
  p.Hi = Hi;
  p.Wi = Wi;
  p.crop = crop;
  p.ksh = ksize_of(Wi, Wr);
  p.ksv = ksize_of(Hi, Hr);
  p.off_bv = crop * (2 + p.ksh);
  p.off_kv = p.off_bv + 2 * crop;
  p.tab_ints = table_ints(crop, p.ksh, p.ksv);
  int *bh = tab, *kh = tab + 2 * crop, *bv = tab + p.off_bv, *kv = tab + p.off_kv;
  axis_coeffs(Wi, Wr, left, crop, p.ksh, bh, kh, w);
  axis_coeffs(Hi, Hr, top, crop, p.ksv, bv, kv, w);
  int x1;
  band_rows(bh, 0, crop, p.xlo, x1);
  p.xn = x1 - p.xlo;
  p.raw_pitch = align16(3 * p.xn) + 16;      // a row starts up to 15 bytes into its first 16-byte slot
  // 16-byte groups per strip row odd: the rows that neighbouring output rows start from
  // (one or two rows apart) begin in different halves of the 128-byte bank line
  p.strip_pitch = align16(3 * crop);
  if ((p.strip_pitch / 16) % 2 == 0) p.strip_pitch += 16;
  // largest band whose tables, raw rows and strip fit
  for (int b = crop < kMaxBand ? crop : kMaxBand; b >= 1; --b) {
    const int tab_bytes = 4 * (crop * (2 + p.ksh) + b * (2 + p.ksv));
    p.tab_lds = tab_bytes <= kTabBudget;
    const int T = p.tab_lds ? align16(tab_bytes) : 0;
    int R = kRawRows;
    while (R > 1 && R * p.raw_pitch > kLdsBudget / 4) --R;
    const int rows_fit = (kLdsBudget - T - R * p.raw_pitch) / p.strip_pitch;
    int need = 0;
    for (int r0 = 0; r0 < crop; r0 += b) {
      int y0, y1;
      band_rows(bv, r0, r0 + b < crop ? r0 + b : crop, y0, y1);
      if (y1 - y0 > need) need = y1 - y0;
    }
    if (need > rows_fit && b > 1) continue;
    p.chunked = need > rows_fit;
    p.band = b;
    p.raw_rows = R;
    p.strip_rows = p.chunked ? rows_fit : need;
    p.lds_raw = T;
    break;
  }
  p.nbands = (crop + p.band - 1) / p.band;
  p.lds_strip = p.lds_raw + p.raw_rows * p.raw_pitch;
  p.lds_bytes = p.lds_strip + p.strip_rows * p.strip_pitch;
  return p;
}

}  // namespace resize
}  // namespace idunno
