// Index math shared by the conv kernels and the host-side checker
// (csrc/tests/host_checks.cpp, built with host ASan + UBSan): block-id remaps and
// the LDS XOR swizzles, the fp16 average pool's thread map and the resize + crop
// geometry.  __host__ __device__ so the checker exercises the exact
// functions the kernels inline, not a re-typed mirror.
#pragma once
#include <hip/hip_runtime.h>

namespace idunno {

// Bijective XCD-aware remap of a linear workgroup id (cdna_hip_programming
// §5 "XCD swizzle must be bijective"): consecutive *logical* tiles land on
// the same XCD so neighbouring tiles share that XCD's L2.
__host__ __device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int nxcd = 8;
  if (nwg < nxcd * 2) return orig;
  const int q = nwg / nxcd, r = nwg % nxcd;
  const int xcd = orig % nxcd, idx = orig / nxcd;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// conv_glds: 16-byte chunk XOR per LDS row; cpr = chunks per row (8: 128-byte
// rows, BK = 64; 4: 64-byte rows, BK = 32).
__host__ __device__ __forceinline__ int swz_r(int row, int cpr) {
  if (cpr == 8) return (row >> 1) & 7;
  const int q = (row >> 2) & 3;
  return (0x78 >> (2 * q)) & 3;
}

// conv_wino_f32: staged raw-input pixel p (64 bytes = 4 chunks of 4 channels) of
// one column-parity half row; a wave's 16 lanes of one channel group read 16
// consecutive pixels -> 16 distinct bank slots per ds_read_b128 lane group.
__host__ __device__ __forceinline__ int wino_raw_swz(int p) { return ((p >> 2) & 1) << 1; }

// conv3x3_c64: 128-byte rows (64 channels)
__host__ __device__ __forceinline__ int c64_swz(int row) { return row & 6; }

// avgpool_kernel (fp16): what thread t of the 256-thread workgroup does for an
// image of cv = C / 8 eight-channel chunks.  It sums pixels g, g + G, ... of
// chunks c8, c8 + stride, ... (< cv); a thread with g >= G idles.  G == 1: the
// thread stores its own chunks.  G > 1 (cv <= 128, one chunk per thread): the G
// partial sums of a chunk meet in LDS and thread g == 0 stores.  cv in (128, 256)
// has room for one group only, so it takes the strided one-group map like
// cv >= 256 (t / cv would put threads cv..255 in a second "group" that owns no
// pixels but still stores).
struct AvgpoolMap {
  int G, g, c8, stride;
};
__host__ __device__ __forceinline__ AvgpoolMap avgpool_map(int t, int cv) {
  if (cv > 128) return {1, 0, t, 256};
  return {256 / cv, t / cv, t % cv, cv};
}

// resize_crop: torchvision's Resize(shorter side -> resize) + CenterCrop(crop)
// geometry.  The crop offset is round-half-even of (n - crop) / 2 on integers
// (Python's round(), as CenterCrop, load_image_u8 and the JPEG path compute it);
// n >= crop.
__host__ __device__ __forceinline__ int center_crop_offset(int n, int crop) {
  const int d = n - crop, h = d / 2;
  return (d & 1) ? h + (h & 1) : h;
}
__host__ __device__ __forceinline__ void resize_crop_geometry(int Hi, int Wi, int resize, int crop, int& Hr,
                                                              int& Wr, int& top, int& left) {
  if (Hi <= Wi) {
    Hr = resize;
    Wr = (int)((long)resize * Wi / Hi);
  } else {
    Wr = resize;
    Hr = (int)((long)resize * Hi / Wi);
  }
  top = center_crop_offset(Hr, crop);
  left = center_crop_offset(Wr, crop);
}

}  // namespace idunno
