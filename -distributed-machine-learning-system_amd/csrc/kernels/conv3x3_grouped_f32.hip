// Grouped 3x3 conv (pad 1, stride 1 or 2) + bias (+ReLU) on fp32 NHWC activations
// for gfx950: the ResNeXt middle conv of the all-f32-MFMA path (HipRunner split =
// False) and of the range-guard rerun.  Products are exact in f32 and accumulation
// is f32 (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain as in conv_f32.hip); there
// is no range guard.  Without this kernel that path runs the dense conv on the
// block-diagonal expansion: groups x the weight bytes and the MFMA work.
//
//   * Channel-block-local GEMM as in conv3x3_grouped.hip (grouped_math.h): CB =
//     max(16, Cg), weights fp32 rows [C][9 * CB], k = tap * CB + ci
//     (models/packed.py pack_grouped_f32_weight; zeros outside an output's own group
//     when Cg < 16).
//   * A workgroup (4 waves) owns a slab of 64 channels x a tile of TH x 16 output
//     pixels (TH = 8 at stride 1, 2 at stride 2), the slab varying slowest in the
//     grid.  It stages the tile's input patch with its halo (10 x 18 pixels, 5 x 33
//     at stride 2; the zero padding and a half slab's missing channels written as
//     zeros) into LDS as fp32 with 16-byte loads and stores: 46,080 / 42,240 bytes.
//   * LDS image: a staged pixel is exactly its 64 channels = 256 bytes = one pass over
//     the 64 banks, as 16 chunks of 4 floats, and NO padding.  Padding cannot
//     serve both strides: a ds_read_b128 lane group is 16 lanes on pixels `stride`
//     apart, and at stride 2 the step between lanes is 2 * pitch dwords, a multiple
//     of 8 for every 16-byte-aligned pitch, so 16 lanes x 4 banks can reach at most
//     32 of the 64 banks (two-way conflicts; conv3x3_grouped.hip's 16-byte pad has
//     them).  Instead chunk q of the pixel in staged column c is stored at chunk
//     q ^ f32_swz(c), f32_swz(c) = (c / stride) & 15.  The 16 lanes of a group read
//     one logical chunk of the pixels in columns col * stride + kx, col = 0 .. 15;
//     c / stride is then col (+ 1 at stride 2's kx = 2), 16 consecutive values, so
//     the 16 XORed chunks are all different: 16 x 4 = 64 distinct banks, at both
//     strides and every tap.  The staging stores are conflict-free as well: 16
//     consecutive lanes write the 16 chunks of one pixel.
//   * Wave w computes output channels [16 w, 16 w + 16) of the slab: one 16 x 16
//     fragment per 16-pixel row of the tile.  conv_f32.hip's fragment trick: one
//     ds_read_b128 gives lane group g = lane >> 4 the channels 4 g .. 4 g + 3 of a
//     16-channel chunk of the lane's pixel at one tap, and four
//     v_mfma_f32_16x16x4_f32 consume elements 0 .. 3 (MFMA t sums channels t, 4 + t,
//     8 + t, 12 + t).  The matching weights of a lane are the four consecutive floats
//     w[row][tap * CB + 16 c + 4 g ..+3]: one 16-byte load per (tap, chunk), 9 * CB / 4
//     = 36 / 72 / 144 VGPRs that stay in registers for the whole tile (no scratch;
//     the resource report is in docs/KERNELS.md).
//   * The tile's rows are walked two at a time: two independent accumulators hide the
//     MFMA's dependent latency.  Both are tied to VGPRs (reg_tie) in the K loop's own
//     basic block, the lesson written up in conv3x3_grouped.hip.
//   * Epilogue: lane (col, kq) holds output channels nb + 4 kq .. + 3 of pixel col:
//     bias, ReLU, one float4 store per lane and row, no lane exchange.  Pixels
//     outside the output are not stored.
#include "../common.h"
#include "../grouped_math.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

struct GroupedF32Args {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int B, H, W, C, Ho, Wo;
  int tiles_x, tiles_y, per_slab;   // per_slab = B * tiles_y * tiles_x
  int relu;
};

template <int STRIDE, int CB>
__global__ void __launch_bounds__(256) conv3x3_grouped_f32_kernel(const GroupedF32Args a) {
  using namespace grouped;
  constexpr int TH = tile_rows(STRIDE), IH = in_rows(STRIDE), IW = in_cols(STRIDE);
  constexpr int NCH = CB / 16;                       // 16-channel chunks (one ds_read_b128, four MFMAs) per tap
  constexpr int WROW = 9 * CB;                       // floats per weight row
  static_assert(TH % 2 == 0 && kSlab % CB == 0 && CB % 16 == 0 && IH * IW * kF32Pixel * 4 <= 65536, "tile shape");
  __shared__ __attribute__((aligned(16))) float patch[IH * IW * kF32Pixel];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kq = lane >> 4;

  // tile index: the channel slab varies slowest (the workgroups in flight share its weights in L2)
  const int t = blockIdx.x;
  const int slab = t / a.per_slab;
  int r = t - slab * a.per_slab;
  const int b = r / (a.tiles_y * a.tiles_x);
  r -= b * a.tiles_y * a.tiles_x;
  const int oy0 = (r / a.tiles_x) * TH, ox0 = (r % a.tiles_x) * kTW;
  const int nch = min(kSlab, a.C - slab * kSlab);    // 64, or 32 in the last slab of a C % 64 == 32 tensor
  const bool active = 16 * wave < nch;               // wave-uniform

  // ---- this wave's weights -> registers: wv[tap][c][t] feeds MFMA t of chunk c ------------
  float4v wv[9][NCH];
  float4v bv = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const float* wrow = a.w + (size_t)(slab * kSlab + 16 * wave + col) * WROW + 4 * kq;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int c = 0; c < NCH; ++c) wv[tap][c] = *reinterpret_cast<const float4v*>(wrow + tap * CB + 16 * c);
    bv = *reinterpret_cast<const float4v*>(a.bias + slab * kSlab + 16 * wave + 4 * kq);
  }

  // ---- stage the input patch (16 bytes per lane; padding pixels and absent channels as zeros) ---
  const int cvalid = nch / 4;                        // chunks of a pixel that exist in memory
  const float* xb = a.x + (size_t)b * a.H * a.W * a.C + (size_t)slab * kSlab;
  constexpr int TOTAL = IH * IW * kF32Chunks, BATCH = 4;
  for (int i0 = tid; i0 < TOTAL; i0 += 256 * BATCH) {
    float4v v[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + 256 * j;
      v[j] = float4v{0.f, 0.f, 0.f, 0.f};
      if (i < TOTAL) {
        const int pix = i / kF32Chunks, ch = i - pix * kF32Chunks;
        const InPixel p = in_pixel(oy0, ox0, STRIDE, pix / IW, pix % IW, a.H, a.W);
        if (p.inside && ch < cvalid)
          v[j] = *reinterpret_cast<const float4v*>(xb + ((size_t)p.iy * a.W + p.ix) * a.C + ch * 4);
      }
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + 256 * j;
      if (i < TOTAL) {
        const int pix = i / kF32Chunks, ch = i - pix * kF32Chunks;
        *reinterpret_cast<float4v*>(patch + f32_lds_off(pix, pix % IW, ch, STRIDE)) = v[j];
      }
    }
  }
  __syncthreads();
  if (!active) return;

  // ---- per-lane B operand offsets (floats from tile row 0): chunk c of tap's pixel for output column col ---
  const int q0 = frag_block_base(CB, wave) / 4 + kq;  // this lane's chunk of the block's first 16 channels
  int boff[9][NCH];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      boff[tap][c] = f32_lds_off(lds_pixel(0, col, tap, STRIDE), col * STRIDE + tap % 3, q0 + 4 * c, STRIDE);
  const int nb = slab * kSlab + 16 * wave;            // first output channel of this wave's fragment
  const int ox = ox0 + col;

  for (int g = 0; g < TH; g += 2) {
    if (oy0 + g >= a.Ho) break;                       // wave-uniform
    const float* rows = patch + g * STRIDE * IW * kF32Pixel;
    float4v acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float4v bx[2];
#pragma unroll
        for (int e = 0; e < 2; ++e)
          bx[e] = *reinterpret_cast<const float4v*>(rows + e * STRIDE * IW * kF32Pixel + boff[tap][c]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int e = 0; e < 2; ++e)
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[tap][c][k], bx[e][k], acc[e], 0, 0, 0);
      }
    }
    // both accumulators leave the MFMA pipeline here, in the K loop's own basic block, where the
    // compiler counts the MFMA -> accumulator-read wait states (conv3x3_grouped.hip)
    reg_tie(acc[0]);
    reg_tie(acc[1]);
    // ---- epilogue: lane (col, kq) holds output channels nb + 4 kq .. + 3 of pixel (oy0 + g + e, ox) ---
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float4v v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[e][i] + bv[i];
        if (a.relu) v[i] = fmaxf(v[i], 0.f);
      }
      if (oy0 + g + e < a.Ho && ox < a.Wo) {
        const size_t m = ((size_t)b * a.Ho + oy0 + g + e) * a.Wo + ox;
        *reinterpret_cast<float4v*>(a.y + m * a.C + nb + 4 * kq) = v;
      }
    }
  }
}

template <int STRIDE>
static void grouped_f32_launch_cb(const GroupedF32Args& a, int cb, int grid, hipStream_t st) {
  if (cb == 16)
    hipLaunchKernelGGL((conv3x3_grouped_f32_kernel<STRIDE, 16>), dim3(grid), dim3(256), 0, st, a);
  else if (cb == 32)
    hipLaunchKernelGGL((conv3x3_grouped_f32_kernel<STRIDE, 32>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv3x3_grouped_f32_kernel<STRIDE, 64>), dim3(grid), dim3(256), 0, st, a);
}

bool conv3x3_grouped_f32_launch(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C,
                                int groups, int stride, int relu, hipStream_t st) {
  using namespace grouped;
  if (!conv3x3_grouped_supported(C, groups, stride)) return false;
  GroupedF32Args a{};
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.y = y;
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.Ho = out_size(H, stride);
  a.Wo = out_size(W, stride);
  a.tiles_x = (a.Wo + kTW - 1) / kTW;
  a.tiles_y = (a.Ho + tile_rows(stride) - 1) / tile_rows(stride);
  a.relu = relu;
  const long per = (long)B * a.tiles_y * a.tiles_x, total = per * ((C + kSlab - 1) / kSlab);
  if (total <= 0 || total >= (1L << 31)) return false;
  a.per_slab = (int)per;
  const int cb = block_of(C / groups), grid = (int)total;
  if (stride == 1) grouped_f32_launch_cb<1>(a, cb, grid, st);
  else grouped_f32_launch_cb<2>(a, cb, grid, st);
  return true;
}

}  // namespace idunno
