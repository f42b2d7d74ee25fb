// resize_crop_u8: uint8 [B, Hi, Wi, 3] -> uint8 [B, crop, crop, 3], Pillow's
// Image.resize(..., BILINEAR) of the shorter side to `resize` + centre crop, in Pillow's own
// 8-bit fixed-point arithmetic (csrc/resize_math.h builds the tables on the host), as a
// separable two-pass kernel in one launch.
//
// Work split: one 256-thread workgroup = one image x one band of output rows (Plan::band,
// at most 16).  It reads only the input rows the band's vertical taps touch and only the
// input columns the crop's horizontal taps touch -- the crop is in the tables.
//
// Per workgroup, LDS = [tables | raw rows | strip]:
//   tables  the horizontal bounds / weights of all crop columns and the band's slice of the
//           vertical ones (when they fit kTabBudget; else both are read from memory);
//   raw     up to kRawRows input rows at a time, copied with 16-byte loads.  A row starts at
//           an arbitrary byte, so it is staged at its offset within its first 16-byte slot:
//           whole slots inside the row move as uint4, the head and tail slots byte by byte;
//   strip   pass 1's output [input row][x][c], 8-bit: the horizontal filter accumulated in
//           32 bits from 1 << (PRECISION_BITS - 1), shifted and clipped, as
//           ImagingResampleHorizontal_8bpc leaves it.  Rows are strip_pitch bytes apart (an odd
//           number of 16-byte groups).
// Pass 1: a thread filters one (row, x) pixel, three channels against one weight per tap.
// Pass 2: a thread owns 16 consecutive bytes of an output row: per vertical tap one 16-byte
// LDS read and 16 multiply-adds, then shift, clip and one 16-byte store (byte stores where
// the row's end or an unaligned `out` does not allow it).
//
// A band of one row whose input rows do not fit the strip (supports beyond ~29 input pixels
// at crop 256) is `chunked`: the rows pass through the strip strip_rows at a time and the 16
// accumulators stay in registers between chunks; integer sums do not care about the order.
//
// No matrix instructions (a byte-bandwidth kernel), no scratch, plain C++ stores only.
#include "../common.h"
#include "../kernels.h"
#include "../resize_math.h"

namespace idunno {

using resize::Plan;

namespace {

__device__ __forceinline__ unsigned clip8(int v) {
  v >>= resize::kPrecisionBits;
  return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// first byte of columns [xlo, ..) of input row y of image b
__device__ __forceinline__ const uint8_t* row_src(const uint8_t* img, const Plan& p, int b, int y) {
  return img + (((size_t)b * p.Hi + y) * p.Wi + p.xlo) * 3;
}

// Input rows [ys, ye) -> strip rows 0 .. ye - ys: staged raw_rows at a time, then pass 1.
__device__ __forceinline__ void fill_strip(const uint8_t* __restrict__ img, const Plan& p, int b, int ys, int ye,
                                           const int* bh, const int* kh, uint8_t* raw, uint8_t* strip) {
  const int tid = threadIdx.x;
  const int nvec = p.raw_pitch >> 4, nbytes = 3 * p.xn;
  for (int yr = ys; yr < ye; yr += p.raw_rows) {
    const int n = min(p.raw_rows, ye - yr);
    __syncthreads();                        // the previous step's readers of raw (and of the strip) are done
    for (int i = tid; i < n * nvec; i += resize::kThreads) {
      const int row = i / nvec, v = i - row * nvec;
      const uint8_t* src = row_src(img, p, b, yr + row);
      const int head = (int)((uintptr_t)src & 15);
      const resize::RawSlot s = resize::raw_slot(head, v, nbytes);
      uint8_t* dst = raw + row * p.raw_pitch + 16 * v;
      if (s.whole) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src + s.lo);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (s.lo + j >= 0 && s.lo + j < nbytes) dst[j] = src[s.lo + j];
      }
    }
    __syncthreads();
    for (int i = tid; i < n * p.crop; i += resize::kThreads) {
      const int row = i / p.crop, x = i - row * p.crop;
      const int head = (int)((uintptr_t)row_src(img, p, b, yr + row) & 15);
      const uint8_t* rp = raw + row * p.raw_pitch + head + 3 * (bh[2 * x] - p.xlo);
      const int nt = bh[2 * x + 1];
      const int* k = kh + x * p.ksh;
      int a0 = 1 << (resize::kPrecisionBits - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < nt; ++t) {
        const int kk = k[t];
        a0 += (int)rp[3 * t] * kk;
        a1 += (int)rp[3 * t + 1] * kk;
        a2 += (int)rp[3 * t + 2] * kk;
      }
      uint8_t* sp = strip + (yr - ys + row) * p.strip_pitch + 3 * x;
      sp[0] = (uint8_t)clip8(a0);
      sp[1] = (uint8_t)clip8(a1);
      sp[2] = (uint8_t)clip8(a2);
    }
  }
  __syncthreads();
}

// Pass 2 of output row r (band-relative), bytes [16 g, 16 g + 16): adds the taps that lie in
// input rows [ys, ye), which are strip rows 0 .. ye - ys.
__device__ __forceinline__ void vertical_taps(const Plan& p, const int* bv, const int* kv, const uint8_t* strip, int r,
                                              int g, int ys, int ye, int (&acc)[16]) {
  const int ymin = bv[2 * r], nt = bv[2 * r + 1];
  const int t0 = max(0, ys - ymin), t1 = min(nt, ye - ymin);
  const int* k = kv + r * p.ksv;
  const uint8_t* sp = strip + (ymin + t0 - ys) * p.strip_pitch + 16 * g;
  for (int t = t0; t < t1; ++t, sp += p.strip_pitch) {
    const uint4 q = *reinterpret_cast<const uint4*>(sp);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    const int kk = k[t];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += (int)((w[j >> 2] >> (8 * (j & 3))) & 255u) * kk;
  }
}

__device__ __forceinline__ void store16(uint8_t* __restrict__ out, const Plan& p, int b, int row, int g,
                                        const int (&acc)[16]) {
  const int rowbytes = 3 * p.crop;
  uint8_t* o = out + ((size_t)b * p.crop + row) * rowbytes + 16 * g;
  unsigned w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    w[q] = clip8(acc[4 * q]) | clip8(acc[4 * q + 1]) << 8 | clip8(acc[4 * q + 2]) << 16 | clip8(acc[4 * q + 3]) << 24;
  if (16 * g + 16 <= rowbytes && ((uintptr_t)o & 15) == 0) {
    *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (16 * g + j < rowbytes) o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

}  // namespace

template <bool kTabLds>
__global__ __launch_bounds__(resize::kThreads) void resize_crop_u8_kernel(const uint8_t* __restrict__ img,
                                                                          uint8_t* __restrict__ out,
                                                                          const int* __restrict__ tab, const Plan p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.nbands, r0 = (blockIdx.x - b * p.nbands) * p.band;
  const int nr = min(p.band, p.crop - r0);
  const int *bh = tab, *kh = tab + 2 * p.crop, *bv = tab + p.off_bv + 2 * r0, *kv = tab + p.off_kv + r0 * p.ksv;
  if (kTabLds) {
    // the horizontal tables whole, the vertical ones for this band's rows
    int* s = reinterpret_cast<int*>(smem);
    for (int i = tid; i < p.off_bv; i += resize::kThreads) s[i] = tab[i];
    for (int i = tid; i < 2 * nr; i += resize::kThreads) s[p.off_bv + i] = bv[i];
    for (int i = tid; i < nr * p.ksv; i += resize::kThreads) s[p.off_bv + 2 * p.band + i] = kv[i];
    bh = s;
    kh = s + 2 * p.crop;
    bv = s + p.off_bv;
    kv = bv + 2 * p.band;
    __syncthreads();
  }
  uint8_t* raw = smem + p.lds_raw;
  uint8_t* strip = smem + p.lds_strip;
  int y0, y1;
  resize::band_rows(bv, 0, nr, y0, y1);
  const int G = (3 * p.crop + 15) >> 4, items = nr * G;   // 16-byte groups per output row, in the band
  if (!p.chunked) {
    fill_strip(img, p, b, y0, y1, bh, kh, raw, strip);
    for (int it = tid; it < items; it += resize::kThreads) {
      const int r = it / G, g = it - r * G;
      int acc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 1 << (resize::kPrecisionBits - 1);
      vertical_taps(p, bv, kv, strip, r, g, y0, y1, acc);
      store16(out, p, b, r0 + r, g, acc);
    }
    return;
  }
  // one output row (items = G <= 48 threads in pass 2), its input rows strip_rows at a time
  int acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 1 << (resize::kPrecisionBits - 1);
  for (int ys = y0; ys < y1; ys += p.strip_rows) {
    const int ye = min(ys + p.strip_rows, y1);
    fill_strip(img, p, b, ys, ye, bh, kh, raw, strip);
    if (tid < items) vertical_taps(p, bv, kv, strip, 0, tid, ys, ye, acc);
  }
  if (tid < items) store16(out, p, b, r0, tid, acc);
}

void resize_crop_u8_launch(const uint8_t* img, uint8_t* out, const int* tab, const Plan& p, int B, hipStream_t st) {
  if (B <= 0) return;
  const dim3 grid((unsigned)((size_t)B * p.nbands));
  if (p.tab_lds)
    hipLaunchKernelGGL(resize_crop_u8_kernel<true>, grid, dim3(resize::kThreads), p.lds_bytes, st, img, out, tab, p);
  else
    hipLaunchKernelGGL(resize_crop_u8_kernel<false>, grid, dim3(resize::kThreads), p.lds_bytes, st, img, out, tab, p);
}

}  // namespace idunno
