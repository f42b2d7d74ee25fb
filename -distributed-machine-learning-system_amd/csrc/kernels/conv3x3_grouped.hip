// Grouped 3x3 conv (pad 1, stride 1 or 2) + bias (+ReLU) for gfx950: the middle
// conv of a ResNeXt bottleneck (32 groups of Cg = 4 .. 64 channels).
//
// The conv is memory-bound (its FLOPs are the dense conv's / groups), so the kernel
// is built to read every activation byte from HBM once and write every output byte
// once; the MFMA runs far below its rate and that is fine.
//
//   * A grouped conv is channel-block-local (grouped_math.h): with CB = max(16, Cg)
//     output channels [CB j, CB j + CB) read input channels of the same range.  The
//     weights are [Cout][9 * CB] halfs, K = tap * CB + ci (models/packed.py
//     pack_grouped_weight; zeros outside an output's group when Cg < 16); the split
//     form is [Cout][hi 9 * CB | lo 9 * CB] (pack_grouped_split_weight).
//   * A workgroup (4 waves) owns a slab of 64 channels x a tile of TH x 16 output
//     pixels (TH = 8 at stride 1, 2 at stride 2).  It stages the tile's input patch
//     (halo included, the zero padding written as zeros) for its 64 channels into LDS
//     with 16-byte loads and stores; a staged pixel is its 64 channels (split: 128
//     halfs [hi x32][lo x32] twice) + 8 halfs of padding.
//   * Wave w computes the slab's output channels [16 w, 16 w + 16): ONE 16-output
//     MFMA fragment whose weights (ksteps(CB) = 5 / 9 / 18 A operands, twice that in
//     the split form) stay in registers for the whole tile.  It walks the tile's
//     rows two at a time: per K-step one ds_read_b128 per row (B operand: 8 channels
//     of one tap of one pixel) and one v_mfma_f32_16x16x32_f16 (split: hi*lo + lo*hi
//     + hi*hi, f32 accumulation, times acc_scale).
//   * Epilogue: bias, ReLU; fp16: the two rows' fragments trade halves
//     (split_swap_out) so that a lane stores 8 consecutive channels of one pixel;
//     split: hi/lo of a fragment trade the same way.  16-byte stores either way.
//     The split form raises the range-guard flag like every split epilogue.
#include "../common.h"
#include "../grouped_math.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

struct GroupedArgs {
  const half_t* x;
  const half_t* w;
  const float* bias;
  half_t* y;
  int B, H, W, C, Ho, Wo;
  int tiles_x, tiles_y, per_slab;   // per_slab = B * tiles_y * tiles_x
  int relu;
  float acc_scale;
  int* ovf;
};

template <bool SPLIT, int STRIDE, int CB>
__global__ void __launch_bounds__(256) conv3x3_grouped_kernel(const GroupedArgs a) {
  using namespace grouped;
  constexpr int TH = tile_rows(STRIDE), IH = in_rows(STRIDE), IW = in_cols(STRIDE);
  constexpr int PIXH = (SPLIT ? 2 : 1) * kSlab;      // halfs of a pixel's slab channels
  constexpr int PITCH = lds_pitch(SPLIT);
  constexpr int CPP = PIXH / 8;                      // 16-byte chunks per staged pixel
  constexpr int KS = ksteps(CB);
  static_assert(TH % 2 == 0 && kSlab % CB == 0 && IH * IW * PITCH * 2 <= 65536, "tile shape");
  constexpr int WROW = (SPLIT ? 2 : 1) * 9 * CB;     // halfs per weight row
  __shared__ __attribute__((aligned(16))) half_t patch[IH * IW * PITCH];

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
  const int cpix = (SPLIT ? 2 : 1) * a.C;            // halfs per global pixel
  const bool active = 16 * wave < nch;               // wave-uniform

  // ---- this wave's weights -> registers ----------------------------------------------
  half8v wh[KS], wl[SPLIT ? KS : 1];
  float4v bv = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const half_t* wrow = a.w + (size_t)(slab * kSlab + 16 * wave + col) * WROW;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int kk = 32 * s + 8 * kq;
      half8v h = {0, 0, 0, 0, 0, 0, 0, 0}, l = h;
      if (kk < 9 * CB) {
        h = *reinterpret_cast<const half8v*>(wrow + kk);
        if constexpr (SPLIT) l = *reinterpret_cast<const half8v*>(wrow + 9 * CB + kk);
      }
      wh[s] = h;
      if constexpr (SPLIT) wl[s] = l;
    }
    bv = *reinterpret_cast<const float4v*>(a.bias + slab * kSlab + 16 * wave + 4 * kq);
  }

  // ---- stage the input patch (16 bytes per lane; padding pixels as zeros) ---------------
  const int cvalid = nch * (SPLIT ? 2 : 1) / 8;      // chunks of a pixel that exist in memory
  const half_t* xb = a.x + (size_t)b * a.H * a.W * cpix + (size_t)slab * PIXH;
  constexpr int TOTAL = IH * IW * CPP, BATCH = 4;
  for (int i0 = tid; i0 < TOTAL; i0 += 256 * BATCH) {
    vec16 v[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + 256 * j;
      v[j] = zero16();
      if (i < TOTAL) {
        const int pix = i / CPP, ch = i - pix * CPP;
        const InPixel p = in_pixel(oy0, ox0, STRIDE, pix / IW, pix % IW, a.H, a.W);
        if (p.inside && ch < cvalid)
          v[j] = *reinterpret_cast<const vec16*>(xb + ((size_t)p.iy * a.W + p.ix) * cpix + ch * 8);
      }
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + 256 * j;
      if (i < TOTAL) {
        const int pix = i / CPP, ch = i - pix * CPP;
        *reinterpret_cast<vec16*>(patch + pix * PITCH + ch * 8) = v[j];
      }
    }
  }
  __syncthreads();
  if (!active) return;

  // ---- per-lane B operand offsets: K-step s reads 8 channels of tap(s) at the lane's pixel ---
  const int bbase = frag_block_base(CB, wave);
  int boff[KS];                                      // halfs from output pixel (0, 0)'s tap-0 staged pixel
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const KSlot k = kslot(CB, 32 * s + 8 * kq);
    boff[s] = k.tap < 9 ? lds_pixel(0, col, k.tap, STRIDE) * PITCH + chan_off(SPLIT, bbase + k.ci) : -1;
  }
  const int nb = slab * kSlab + 16 * wave;           // first output channel of this wave's fragment
  const int ox = ox0 + col;

  for (int g = 0; g < TH; g += 2) {
    if (oy0 + g >= a.Ho) break;                      // wave-uniform
    float4v acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        half8v bh = {0, 0, 0, 0, 0, 0, 0, 0}, bl = bh;
        if (boff[s] >= 0) {
          const half_t* src = patch + (g + e) * STRIDE * IW * PITCH + boff[s];
          bh = *reinterpret_cast<const half8v*>(src);
          if constexpr (SPLIT) bl = *reinterpret_cast<const half8v*>(src + 32);
        }
        if constexpr (SPLIT) {
          acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], bl, acc[e], 0, 0, 0);
          acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[s], bh, acc[e], 0, 0, 0);
        }
        acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], bh, acc[e], 0, 0, 0);
      }
    }
    // Both accumulators leave the MFMA pipeline HERE, in the K loop's own basic block, where hipcc
    // counts the MFMA -> accumulator-read wait states.  Left to the epilogue, the second row's read
    // landed behind the first row's range-guard branch, and on the branch's short side (no guard
    // flag set) element 3 was read before the last MFMA had written it: one tap's hi*hi term missing.
    reg_tie(acc[0]);
    reg_tie(acc[1]);
    // ---- epilogue: lane (col, kq) holds output channels nb + 4 kq .. + 3 of pixel (oy0 + g + e, ox) ---
    bool ok[2];
    float4v v[2];
    half4v oh[2], ol[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      ok[e] = oy0 + g + e < a.Ho && ox < a.Wo;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[e][i] = acc[e][i] * (SPLIT ? a.acc_scale : 1.f) + bv[i];
        if (a.relu) v[e][i] = fmaxf(v[e][i], 0.f);
        if (!ok[e]) v[e][i] = 0.f;                   // a pixel outside the output: nothing to guard or store
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if constexpr (SPLIT) {
        split_guard(a.ovf, v[e]);
        split_f16x4(v[e], oh[e], ol[e]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) oh[e][i] = (half_t)v[e][i];
      }
    }
    if constexpr (SPLIT) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const u32x4_sw o = split_swap_out(oh[e], ol[e]);   // every lane swaps
        if (ok[e]) {
          const size_t m = ((size_t)b * a.Ho + oy0 + g + e) * a.Wo + ox;
          *reinterpret_cast<u32x4_sw*>(a.y + m * cpix + split_off_q(nb, kq)) = o;
        }
      }
    } else {
      // kq even: row g's channels nb + 8 (kq / 2) .. + 7; kq odd: row g + 1's
      const u32x4_sw o = split_swap_out(oh[0], oh[1]);     // every lane swaps
      const int e = kq & 1;
      if (ok[e]) {
        const size_t m = ((size_t)b * a.Ho + oy0 + g + e) * a.Wo + ox;
        *reinterpret_cast<u32x4_sw*>(a.y + m * cpix + nb + 8 * (kq >> 1)) = o;
      }
    }
  }
}

bool conv3x3_grouped_supported(int C, int groups, int stride) {
  return C > 0 && groups > 1 && C % 32 == 0 && C % groups == 0 && grouped::cg_ok(C / groups) &&
         (stride == 1 || stride == 2);
}

template <bool SPLIT, int STRIDE>
static void grouped_launch_cb(const GroupedArgs& a, int cb, int grid, hipStream_t st) {
  if (cb == 16)
    hipLaunchKernelGGL((conv3x3_grouped_kernel<SPLIT, STRIDE, 16>), dim3(grid), dim3(256), 0, st, a);
  else if (cb == 32)
    hipLaunchKernelGGL((conv3x3_grouped_kernel<SPLIT, STRIDE, 32>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv3x3_grouped_kernel<SPLIT, STRIDE, 64>), dim3(grid), dim3(256), 0, st, a);
}

bool conv3x3_grouped_launch(const half_t* x, const half_t* w, const float* bias, half_t* y, int B, int H, int W, int C,
                            int groups, int stride, int relu, bool split, float acc_scale, int* ovf, hipStream_t st) {
  using namespace grouped;
  if (!conv3x3_grouped_supported(C, groups, stride)) return false;
  GroupedArgs a{};
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
  a.acc_scale = acc_scale;
  a.ovf = split ? ovf : nullptr;
  const long per = (long)B * a.tiles_y * a.tiles_x, total = per * ((C + kSlab - 1) / kSlab);
  if (total <= 0 || total >= (1L << 31)) return false;
  a.per_slab = (int)per;
  const int cb = block_of(C / groups), grid = (int)total;
  if (split) {
    if (stride == 1) grouped_launch_cb<true, 1>(a, cb, grid, st);
    else grouped_launch_cb<true, 2>(a, cb, grid, st);
  } else {
    if (stride == 1) grouped_launch_cb<false, 1>(a, cb, grid, st);
    else grouped_launch_cb<false, 2>(a, cb, grid, st);
  }
  return true;
}

}  // namespace idunno
