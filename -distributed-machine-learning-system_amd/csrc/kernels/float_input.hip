// Normalised float images -> the stem operands the uint8 producers write
// (preprocess, preprocess_pack3, preprocess_pack3_split), so a batch that is
// already normalised (fp32 or fp16, NCHW or channels-last, possibly a batch
// view) enters the HIP path without going back to bytes.
//
// One workgroup (4 waves) = one band of fi_band_rows(W) rows of one image; one
// launch per batch.
//   1. Stage.  A wave takes whole source segments -- a channels-last row (3W
//      contiguous elements) or one plane's row of an NCHW image (W elements) --
//      and its lanes take the segment's 16-byte vectors (float_input_math.h
//      fi_item: the elements before the first 16-byte boundary and after the last
//      are loaded one by one, so a row may start anywhere).  The values go to
//      LDS as fp32 words, interleaved (word 3x + ch) and padded by fi_phys.
//   2. Write.  A wave takes whole destination rows (an nhwc4 row; one copy of a
//      packed row), its lanes the row's 16-byte slots: the lane gathers the
//      slot's words from LDS (padding positions are zeros made in registers, so
//      no memset precedes the launch), rounds or splits them, and stores 16 bytes.
// Both sides of memory see consecutive lanes on consecutive 16 bytes; the
// strided side is the LDS, whose padding keeps every access conflict-free.
// The values are copied: fp32 -> fp32 bit for bit, -> fp16 round-to-nearest-
// even, split hi = fp16(v), lo = fp16(v - hi) with the range guard of the other
// split producers (common.h split_guard).
#include <type_traits>

#include "../float_input_math.h"
#include "../kernels.h"

namespace idunno {

template <typename TI>
__device__ __forceinline__ void fi_stage_vec(const TI* p, float* row, int lo, int ch) {
  if constexpr (sizeof(TI) == 4) {
    const float4v v = *reinterpret_cast<const float4v*>(p + lo);
#pragma unroll
    for (int i = 0; i < 4; ++i) row[fi_phys(fi_seg_word(lo + i, ch))] = v[i];
  } else {
    const half8v v = *reinterpret_cast<const half8v*>(p + lo);
#pragma unroll
    for (int i = 0; i < 8; ++i) row[fi_phys(fi_seg_word(lo + i, ch))] = (float)v[i];
  }
}

// TI: source element (float / half_t).  CL: channels-last source.
template <typename TI, int FORM, bool CL>
__global__ void __launch_bounds__(kFiThreads) float_input_kernel(const FloatInArgs a) {
  extern __shared__ float fi_lds[];
  constexpr int VE = 16 / (int)sizeof(TI);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  constexpr int NWAVE = kFiThreads / kWave;
  const int b = blockIdx.x / a.nbands;
  int y0, nr;
  fi_band(blockIdx.x % a.nbands, a.rows, a.H, y0, nr);
  const int W = a.W, pitch = fi_pitch(W);
  const TI* img = reinterpret_cast<const TI*>(a.src) + (long long)b * a.sb;

  // ---- 1. stage the band ----
  const int n = CL ? 3 * W : W;
  for (int s = wave; s < (CL ? nr : 3 * nr); s += NWAVE) {
    const int r = CL ? s : s / 3, ch = CL ? -1 : s % 3;
    const TI* p = img + (long long)(y0 + r) * a.sh + (CL ? 0 : ch * a.sc);
    float* row = fi_lds + r * pitch;
    const int head = fi_head((unsigned long long)reinterpret_cast<uintptr_t>(p), (int)sizeof(TI), n);
    const int items = fi_items(n, head, VE);
    for (int t = lane; t < items; t += kWave) {
      int lo, hi;
      fi_item(t, n, head, VE, lo, hi);
      if (hi - lo == VE) {
        fi_stage_vec<TI>(p, row, lo, ch);
      } else {
        for (int e = lo; e < hi; ++e) row[fi_phys(fi_seg_word(e, ch))] = (float)p[e];
      }
    }
  }
  __syncthreads();

  // ---- 2. write the operand ----
  if constexpr (FORM == kFiNhwc4F32) {
    for (int r = wave; r < nr; r += NWAVE) {
      const float* row = fi_lds + r * pitch;
      float4v* o = reinterpret_cast<float4v*>(a.out) + ((b * a.H + y0 + r) * W);
      for (int x = lane; x < W; x += kWave)
        o[x] = float4v{row[fi_phys(3 * x)], row[fi_phys(3 * x + 1)], row[fi_phys(3 * x + 2)], 0.f};
    }
  } else if constexpr (FORM == kFiNhwc4F16) {
    for (int r = wave; r < nr; r += NWAVE) {
      const float* row = fi_lds + r * pitch;
      const int p0 = (b * a.H + y0 + r) * W, par = p0 & 1;
      half4v* o = reinterpret_cast<half4v*>(a.out) + p0;
      const int items = fi_pair_items(W, par);
      for (int k = lane; k < items; k += kWave) {
        int x0, x1;
        fi_pair(k, par, W, x0, x1);
        half8v v;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int x = x0 + q < W ? x0 + q : x0;      // a clipped item reads its one pixel twice
#pragma unroll
          for (int c = 0; c < 3; ++c) v[4 * q + c] = (half_t)row[fi_phys(3 * x + c)];
          v[4 * q + 3] = (half_t)0.f;
        }
        if (x1 - x0 == 2)
          *reinterpret_cast<half8v*>(o + x0) = v;      // pixel p0 + x0 is even: 16-byte aligned
        else
          o[x0] = half4v{v[0], v[1], v[2], v[3]};
      }
    }
  } else {
    typedef typename std::conditional<FORM == kFiPack3F32, float, half_t>::type TO;
    constexpr int E = 16 / (int)sizeof(TO);
    constexpr bool SPLIT = FORM == kFiPack3Split;
    const int g = E / a.nc, chunks = a.wp / E, copies = SPLIT ? 2 : 1;
    bool ovf = false;
    for (int rc = wave; rc < nr * a.nc; rc += NWAVE) {
      const int r = rc / a.nc, c = rc % a.nc;
      const float* row = fi_lds + r * pitch;
      TO* o = reinterpret_cast<TO*>(a.out) + ((b * a.H + y0 + r) * copies * a.nc + c) * a.wp;
      for (int j = lane; j < chunks; j += kWave) {
        float v[E];
#pragma unroll
        for (int i = 0; i < E; ++i) {
          const int w = pack3_live_word(E * j + i, c, g, a.pad, W);
          v[i] = w >= 0 ? row[fi_phys(w)] : 0.f;
        }
        if constexpr (FORM == kFiPack3F32) {
          *reinterpret_cast<float4v*>(o + E * j) = float4v{v[0], v[1], v[2], v[3]};
        } else {
          half8v h, l;
#pragma unroll
          for (int i = 0; i < E; ++i) {
            h[i] = (half_t)v[i];
            l[i] = (half_t)(v[i] - (float)h[i]);
            ovf |= !(fabsf(v[i]) < 65504.f);
          }
          *reinterpret_cast<half8v*>(o + E * j) = h;
          if constexpr (SPLIT) *reinterpret_cast<half8v*>(o + a.nc * a.wp + E * j) = l;
        }
      }
    }
    if (SPLIT && a.guard != nullptr && ovf) *a.guard = 1;
  }
}

template <typename TI, bool CL>
static void fi_launch(const FloatInArgs& a, FloatInForm form, hipStream_t st) {
  const dim3 grid((unsigned)(a.B * a.nbands)), block(kFiThreads);
  const size_t lds = (size_t)a.rows * fi_pitch(a.W) * sizeof(float);
  auto kern = form == kFiNhwc4F16   ? float_input_kernel<TI, kFiNhwc4F16, CL>
              : form == kFiNhwc4F32 ? float_input_kernel<TI, kFiNhwc4F32, CL>
              : form == kFiPack3F32 ? float_input_kernel<TI, kFiPack3F32, CL>
              : form == kFiPack3F16 ? float_input_kernel<TI, kFiPack3F16, CL>
                                    : float_input_kernel<TI, kFiPack3Split, CL>;
  hipLaunchKernelGGL(kern, grid, block, lds, st, a);
}

void float_input_launch(const FloatInArgs& a, bool src_f16, bool channels_last, FloatInForm form, hipStream_t st) {
  if (src_f16)
    channels_last ? fi_launch<half_t, true>(a, form, st) : fi_launch<half_t, false>(a, form, st);
  else
    channels_last ? fi_launch<float, true>(a, form, st) : fi_launch<float, false>(a, form, st);
}

}  // namespace idunno
