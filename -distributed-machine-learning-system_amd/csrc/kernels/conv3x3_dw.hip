// Depthwise 3x3 conv (pad 1, stride 1 or 2) + bias (+ReLU / ReLU6) on NHWC fp16 or fp32
// activations for gfx950: the middle conv of MobileNetV2's inverted residuals.
//
// Nine MACs per output and no reduction over channels: there is nothing for a matrix
// instruction to do, and the kernel is a byte mover.  The design goal is that every input
// element leaves HBM once and every output is written once, all in 16-byte accesses.
//
//   * A lane owns one 16-byte channel vector (8 halfs / 4 floats) of one output column of
//     one image and walks a band of output rows downwards.  The flat lane index runs over
//     (image, output column, channel vector) with the channel vector fastest, so the 64
//     lanes of a wave read whole contiguous runs of a pixel row, whatever C is (C = 32
//     halfs is four lanes a pixel), and a workgroup is full for every C and W: the last
//     workgroup of a band is the only ragged one.
//   * Vertical reuse is a rolling three-row window in registers: each step down loads one
//     new input row (two at stride 2: the rows stride 2 never needs are never read) as the
//     lane's three columns, 3 x 16 bytes, and the two older rows shift.  Horizontal reuse
//     is the three loads themselves: in one load instruction the wave's lanes read one
//     contiguous run, and the other two read the same run shifted by a pixel, which the
//     vector L1 serves (3 x the input through a 64 B / clk L1 is far below its rate at
//     HBM speed).  LDS would add a barrier and a second copy for the same bytes.
//   * The nine weight vectors (tap-major [9, C]: one 16-byte load a tap) and the bias stay
//     in registers for the whole band, in the activations' own precision; products are
//     formed in f32 (a half x half product is exact there) and accumulated in f32.
//   * Borders are predication: a tap outside the image is a zero vector, never a load.
//   * Bands: 16 output rows (8 at stride 2), cut evenly; the band index varies fastest in
//     the grid, so the one or two halo rows two bands share are read by workgroups that
//     run together and meet in L2.  At H <= 16 there is one band and no halo at all.
//   * ``clamp_in`` applies min(x, 6) to every loaded value: the ReLU6 of a producer that
//     only has a ReLU epilogue (MobileNetV2's stem runs on the small-C conv kernels).
#include "../common.h"
#include "../kernels.h"

namespace idunno {

struct DwArgs {
  const void* x;
  const void* w;        // [9, C] in x's dtype
  const float* bias;    // [C]
  void* y;
  int B, H, W, C, Ho, Wo;
  int th, nbands;       // output rows per band, bands per image
  int total;            // B * Wo * (C / E) lanes per band
  int act, clamp_in;
};

template <typename T>
struct DwVec;
template <>
struct DwVec<half_t> {
  typedef half8v type;
};
template <>
struct DwVec<float> {
  typedef float4v type;
};

template <typename T, int S>
__global__ void __launch_bounds__(256) conv3x3_dw_kernel(const DwArgs a) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename DwVec<T>::type V;
  const int blk = blockIdx.x;
  const int band = blk % a.nbands;
  const int idx = (blk / a.nbands) * 256 + (int)threadIdx.x;
  if (idx >= a.total) return;
  const int cvs = a.C / E;
  const int cv = idx % cvs;
  const int t = idx / cvs;
  const int ox = t % a.Wo, b = t / a.Wo;
  const int oy0 = band * a.th, oy1 = min(a.Ho, oy0 + a.th);
  const int C = a.C, H = a.H, W = a.W;

  const T* wp = static_cast<const T*>(a.w) + cv * E;
  V wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = *reinterpret_cast<const V*>(wp + (size_t)k * C);
  float bv[E];
#pragma unroll
  for (int e = 0; e < E; e += 4) {
    const float4v q = *reinterpret_cast<const float4v*>(a.bias + cv * E + e);
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[e + i] = q[i];
  }

  const T* xb = static_cast<const T*>(a.x) + (size_t)b * H * W * C + cv * E;
  T* yb = static_cast<T*>(a.y) + (size_t)b * a.Ho * a.Wo * C + cv * E;
  const int ix0 = ox * S - 1;
  const bool cok0 = ix0 >= 0, cok2 = ix0 + 2 < W;       // the centre column ix0 + 1 = ox * S is always inside
  const bool clamp = a.clamp_in != 0;

  auto load_row = [&](int iy, V (&r)[3]) {
    V z;
#pragma unroll
    for (int e = 0; e < E; ++e) z[e] = (T)0.f;
    r[0] = z;
    r[1] = z;
    r[2] = z;
    if (iy < 0 || iy >= H) return;
    const T* p = xb + ((long)iy * W + ix0 + 1) * C;     // the centre column
    if (cok0) r[0] = *reinterpret_cast<const V*>(p - C);
    r[1] = *reinterpret_cast<const V*>(p);
    if (cok2) r[2] = *reinterpret_cast<const V*>(p + C);
    if (clamp) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) r[k][e] = r[k][e] < (T)6.f ? r[k][e] : (T)6.f;
    }
  };

  V r0[3], r1[3], r2[3];
  load_row(oy0 * S - 1, r0);
  if (S == 1) load_row(oy0, r1);
  for (int oy = oy0; oy < oy1; ++oy) {
    if (S == 1) {
      load_row(oy + 1, r2);
    } else {
      load_row(2 * oy, r1);
      load_row(2 * oy + 1, r2);
    }
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = bv[e];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        acc[e] = fmaf((float)r0[kx][e], (float)wv[kx][e], acc[e]);
        acc[e] = fmaf((float)r1[kx][e], (float)wv[3 + kx][e], acc[e]);
        acc[e] = fmaf((float)r2[kx][e], (float)wv[6 + kx][e], acc[e]);
      }
    V o;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float v = acc[e];
      if (a.act) v = fmaxf(v, 0.f);
      if (a.act == 2) v = fminf(v, 6.f);
      o[e] = (T)v;
    }
    *reinterpret_cast<V*>(yb + ((size_t)oy * a.Wo + ox) * C) = o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (S == 1) {
        r0[k] = r1[k];
        r1[k] = r2[k];
      } else {
        r0[k] = r2[k];
      }
    }
  }
}

bool conv3x3_dw_launch(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C,
                       int stride, int act, int clamp_in, bool f32, hipStream_t st) {
  const int E = f32 ? 4 : 8;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % E || (stride != 1 && stride != 2) || act < 0 || act > 2) return false;
  DwArgs a{};
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.y = y;
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.Ho = (H - 1) / stride + 1;
  a.Wo = (W - 1) / stride + 1;
  const int rows = stride == 1 ? 16 : 8;
  a.nbands = (a.Ho + rows - 1) / rows;
  a.th = (a.Ho + a.nbands - 1) / a.nbands;
  const long total = (long)B * a.Wo * (C / E), grid = (total + 255) / 256 * a.nbands;
  if (total >= (1L << 31) || grid >= (1L << 31)) return false;
  a.total = (int)total;
  a.act = act;
  a.clamp_in = clamp_in;
  const dim3 g((unsigned)grid), blk(256);
  if (f32) {
    if (stride == 1) hipLaunchKernelGGL((conv3x3_dw_kernel<float, 1>), g, blk, 0, st, a);
    else hipLaunchKernelGGL((conv3x3_dw_kernel<float, 2>), g, blk, 0, st, a);
  } else {
    if (stride == 1) hipLaunchKernelGGL((conv3x3_dw_kernel<half_t, 1>), g, blk, 0, st, a);
    else hipLaunchKernelGGL((conv3x3_dw_kernel<half_t, 2>), g, blk, 0, st, a);
  }
  return true;
}

}  // namespace idunno
