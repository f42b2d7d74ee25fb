// Shared pieces of the row-streaming split 3x3 64 -> 64 kernels: the one-conv kernel
// (conv3x3_split.hip) and the fused basic-block kernel (conv3x3_split_block.hip).
#pragma once
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

namespace c64s {
constexpr int C = 64;              // channels in and out
constexpr int PIX = 2 * C;         // halfs per pixel (split)
constexpr int RC = 60;             // LDS columns per ring row (W + 2 <= 58 read; 60 = 3.75 whole DMA instructions)
constexpr int RB = RC * 256;       // bytes per ring row
constexpr int RING = 5;            // rows y-2 .. y+1 in use (a row pair's tail fragment) + row y+2 landing
constexpr int BIAS = RING * RB;    // the 64 biases (fp32), read by the epilogue: no VGPRs held for them
constexpr int LDS = BIAS + 256;    // 77,056 B: 2 workgroups per CU
constexpr int WMAX = 56;           // 3 full fragments + an 8-column tail per row
constexpr int NST = 3;             // epilogue stores per wave and row, at least (3 fragments, 16 B a lane)
}  // namespace c64s

struct C64sArgs {
  const half_t* x;      // split [B][H][W][128]
  const half_t* w;      // split weights [64][9 * 128] (pack_split_weight)
  const float* bias;    // [64]
  const half_t* res;    // split [B][H][W][128] or nullptr
  half_t* y;            // split [B][H][W][128]
  const void* zero;     // unused (padding comes from out-of-range buffer offsets)
  int B, H, W, relu, nrows;
  float acc_scale;
  int* ovf;             // split range guard flag or nullptr (common.h split_guard)
};

__device__ __forceinline__ int c64s_slot(int chunk, int col) { return chunk ^ ((2 * col) & 15); }

// ds_read_b128 with an immediate byte offset (invisible to the wait-count pass, see common.h)
template <int OFF>
__device__ __forceinline__ half8v lds_read_b128_off(uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset range");
  half8v v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// fragment f's read (f = 0..2 of the row: immediate offset 4096 * f; f = 3: the
// tail fragment, whose lanes carry their own row base)
__device__ __forceinline__ half8v lds_read_frag(uint32_t addr, int f) {
  switch (f) {
    case 0: return lds_read_b128_off<0>(addr);
    case 1: return lds_read_b128_off<4096>(addr);
    case 2: return lds_read_b128_off<8192>(addr);
    default: return lds_read_b128_off<0>(addr);
  }
}

// Per-lane buffer offsets of the row DMA (constant for the launch), for a workgroup
// of NT threads: chunk i = r * NT + tid of an LDS ring row is column i / 16, slot
// i % 16, which holds global chunk c64s_slot(slot, col) of pixel col - 1; padding
// columns get an offset past the descriptor (zeros).
template <int NT>
__device__ __forceinline__ void c64s_row_offsets(int W, int tid, uint32_t (&voff)[1024 / NT]) {
#pragma unroll
  for (int r = 0; r < 1024 / NT; ++r) {
    const int i = r * NT + tid;
    const int col = i >> 4, slot = i & 15;
    const int ix = col - 1;
    voff[r] = (unsigned)ix < (unsigned)W ? (uint32_t)(ix * 256 + (c64s_slot(slot, col) << 4)) : 0x80000000u;
  }
}

// DMA input row iy of image b into ring slot rs (zeros outside the image):
// RC * 16 = 960 chunks = 15 wave-wide DMA instructions, so the last wave issues one
// fewer than the others (a wave-uniform split: the counted waits of the kernels only
// need each wave's own DMAs to be older than its epilogue stores).  The row's base
// is the uniform soffset.
template <int NT, typename Rsrc>
__device__ __forceinline__ void c64s_load_row(char* ring, Rsrc x_rsrc, const uint32_t (&voff)[1024 / NT], int H, int W,
                                              int b, int iy, int rs, int tid) {
  using namespace c64s;
  const bool rowv = (unsigned)iy < (unsigned)H;
  const int soff = rowv ? (b * H + iy) * W * 256 : 0;
#pragma unroll
  for (int r = 0; r < 1024 / NT; ++r) {
    if (r * NT + (tid & ~63) >= RC * 16) break;   // chunks 960..1023: past the row (wave-uniform)
    dma_buf16(x_rsrc, ring + rs * RB + (r * NT + (tid & ~63)) * 16, rowv ? voff[r] : 0x80000000u, soff);
  }
}

// D groups of B reads in the register ring: D - 1 groups in flight behind the
// group whose MFMAs issue
template <int N>
__device__ __forceinline__ void c64s_wait_groups() {
  lds_waitcnt<2 * N>();
}

template <int N>
struct c64s_nf {
  static constexpr int value = N;
};

}  // namespace idunno
