// Narrow-channel 1x1 conv + bias (+residual) (+ReLU / ReLU6) on NHWC fp16 or fp32
// activations for gfx950: MobileNetV2's expand and project convs and its last 1x1.
//
//   y[M, N] = act(x[M, K] * w[N, K]^T + bias (+ res)),   M = B H W,   K, N multiples of 8, <= 1280
//
// Both GEMM dimensions are small and ragged (K = 16, 24, 144 ...; N = 24 is 1.5 fragments),
// and every MobileNetV2 layer is bandwidth-bound (docs/KERNELS.md has the arithmetic
// intensities): the design moves each activation byte through HBM once and keeps the MFMA
// work out of the way.
//
//   * fp16 runs on v_mfma_f32_16x16x32_f16, fp32 on v_mfma_f32_16x16x4_f32 with true f32
//     products.  The 32-wide K step (rather than 16x16x16) makes every operand fragment
//     one 16-byte read a lane; what it costs is zero padding of K = 16, 24 and 144 to 32,
//     32 and 160, which exists only in LDS and in the (L2-resident) weights, never in HBM
//     activations.  fp32: one 16-byte read feeds four MFMAs (conv_f32.hip's fragment trick:
//     lane group q holds k = 16 c + 4 q .. + 3, MFMA t consumes element t), K step 16.
//   * A workgroup (4 waves) owns an M tile of 16 MF pixels (MF = 4, 2 or 1: the largest
//     whose tile fits 80 KiB of LDS, two workgroups a CU) and ALL of N.  The tile's rows are
//     staged once, with 16-byte loads and stores, zero-filled from K up to Kp and for the
//     rows past M: the weights' zero pad never multiplies stale LDS contents (NaN x 0 is
//     NaN).  x is therefore read from HBM exactly once, by every layer; N tiling (320 ->
//     1280 is ten passes of 128 channels) re-reads only LDS.
//   * LDS rows are padded by 16 bytes: Kp elements are a multiple of 64 bytes, so the pitch
//     is an odd number of 16-byte slots and the 16 lanes of a ds_read_b128 lane group (16
//     consecutive pixels, one k chunk) fall on 16 different slots of the 64 banks.  The
//     staging stores write consecutive chunks of a row: conflict-free as well.
//   * The 4 waves are WN x WM: WN = 1, 2 or 4 waves over pairs of 16-channel fragments
//     (all four when N > 64), WM = 4 / WN over the tile's M fragments, so that N = 16 ..
//     64 still uses every wave.  A wave walks K once per pair: the pair's two weight
//     fragments of a K step are loaded from L2 into registers (16 bytes a lane, the next
//     step's prefetched under this step's MFMAs) and used for every M fragment of the wave.
//     Weights are <= 0.8 MB; they are the MFMA's A operand, the pixels its B operand, so a
//     lane ends with four consecutive output channels of one pixel (transposed accumulator).
//   * Epilogue: bias, residual, activation in that layout; fp32 stores its float4, fp16
//     trades halves between the pair's fragments (v_permlane16_swap, f16_pair_off) for one
//     16-byte store a lane.  Rows past M and channel chunks past N are predicated off: N is
//     a multiple of 8, so an 8-channel chunk is whole or absent, and outputs are not padded.
//   * MobileNetV3 adds hardswish / hardsigmoid epilogues (act 3 / 4), a hardswish on the
//     residual as it is read (res_act 3: the residual is a stem output whose hardswish its
//     consumers finish) and, as the SCALE instantiations, a squeeze-and-excitation input
//     scale: while a row is staged it is multiplied by its own image's row of
//     in_scale[B, K] (image = row / hw: a tile spans several images at 7 x 7 and 14 x 14),
//     the product rounded to the activations' dtype as the module's ``scale * x`` is.  The
//     scaled tensor never exists in HBM.  The instantiations without SCALE are unchanged.
#include "../common.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

struct PwArgs {
  const void* x;
  const void* w;        // [N, Kp] in x's dtype, zero from K to Kp
  const float* bias;    // [N]
  const void* res;      // [M, N] or null
  void* y;              // [M, N]
  int M, K, Kp, N;
  int ldx;              // elements between pixels of x
  int act;
  int wm;               // waves over M fragments: 1, 2 or 4 (<= MF)
  const void* in_scale; // [M / hw, K] in x's dtype (SCALE instantiations)
  int hw;               // pixels per image
  int res_act;          // 3: hardswish on the residual as read
};

constexpr int kPwLdsBytes = 16 * (1280 * 4 + 16);   // one M fragment of the widest fp32 rows: 80.25 KiB

template <typename T>
struct PwFrag;
template <>
struct PwFrag<half_t> {
  typedef half8v type;
  static __device__ __forceinline__ float4v mma(half8v a, half8v b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct PwFrag<float> {
  typedef float4v type;
  static __device__ __forceinline__ float4v mma(float4v a, float4v b, float4v c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], c, 0, 0, 0);
    return c;
  }
};

__device__ __forceinline__ float pw_act(float v, int act) {
  if (act >= 3) {                                         // 3 hardswish, 4 hardsigmoid
    const float h = fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    return act == 3 ? v * h : h;
  }
  if (act) v = fmaxf(v, 0.f);
  if (act == 2) v = fminf(v, 6.f);
  return v;
}

template <typename T, int MF, bool SCALE>
__global__ void __launch_bounds__(256) conv1x1_narrow_kernel(const PwArgs a) {
  constexpr int E = 16 / (int)sizeof(T);    // elements per 16-byte chunk
  constexpr int KS = 4 * E;                 // K step: four lane groups of one chunk
  constexpr bool F16 = sizeof(T) == 2;
  typedef typename PwFrag<T>::type V;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * (16 * MF);
  const int pitch = a.Kp * (int)sizeof(T) + 16;          // bytes

  // ---- stage the tile's rows: 16 bytes a lane, zeros past K and past M --------------------------
  {
    const int cpr = a.Kp / E, kvc = a.K / E, total = 16 * MF * cpr;
    const T* xb = static_cast<const T*>(a.x);
    constexpr int BATCH = 4;
    for (int i0 = tid; i0 < total; i0 += 256 * BATCH) {
      V v[BATCH];
      int off[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int i = i0 + 256 * j;
#pragma unroll
        for (int e = 0; e < E; ++e) v[j][e] = (T)0.f;
        off[j] = -1;
        if (i < total) {
          const int m = i / cpr, c = i - m * cpr;
          off[j] = m * pitch + c * 16;
          if (m0 + m < a.M && c < kvc) {
            v[j] = *reinterpret_cast<const V*>(xb + (size_t)(m0 + m) * a.ldx + c * E);
            if constexpr (SCALE) {
              const V s = *reinterpret_cast<const V*>(static_cast<const T*>(a.in_scale) +
                                                      (size_t)((m0 + m) / a.hw) * a.K + c * E);
#pragma unroll
              for (int e = 0; e < E; ++e) v[j][e] = (T)((float)v[j][e] * (float)s[e]);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j)
        if (off[j] >= 0) *reinterpret_cast<V*>(smem + off[j]) = v[j];
    }
  }
  __syncthreads();

  const int wmask = a.wm - 1;
  const int wm = wave & wmask, wn = wave / a.wm, WN = 4 / a.wm;
  const int npairs = (a.N + 31) / 32, nks = a.Kp / KS;
  const char* brow = smem + col * pitch + q * 16;         // this lane's pixel row of M fragment 0, k chunk q

  for (int pair = wn; pair < npairs; pair += WN) {        // wave-uniform
    const int nb = pair * 32;
    const bool ok0 = nb + col < a.N, ok1 = nb + 16 + col < a.N;
    const T* w0 = static_cast<const T*>(a.w) + (size_t)(nb + col) * a.Kp + q * E;
    const T* w1 = w0 + (size_t)16 * a.Kp;
    V zero;
#pragma unroll
    for (int e = 0; e < E; ++e) zero[e] = (T)0.f;
    float4v acc[MF][2];
#pragma unroll
    for (int j = 0; j < MF; ++j) acc[j][0] = acc[j][1] = float4v{0.f, 0.f, 0.f, 0.f};

    V a0n = ok0 ? *reinterpret_cast<const V*>(w0) : zero;
    V a1n = ok1 ? *reinterpret_cast<const V*>(w1) : zero;
    for (int ks = 0; ks < nks; ++ks) {
      const V a0 = a0n, a1 = a1n;
      if (ks + 1 < nks) {
        a0n = ok0 ? *reinterpret_cast<const V*>(w0 + (ks + 1) * KS) : zero;
        a1n = ok1 ? *reinterpret_cast<const V*>(w1 + (ks + 1) * KS) : zero;
      }
#pragma unroll
      for (int j = 0; j < MF; ++j) {
        if ((j & wmask) != wm) continue;                  // wave-uniform
        const V bx = *reinterpret_cast<const V*>(brow + 16 * j * pitch + ks * (KS * (int)sizeof(T)));
        acc[j][0] = PwFrag<T>::mma(a0, bx, acc[j][0]);
        acc[j][1] = PwFrag<T>::mma(a1, bx, acc[j][1]);
      }
    }

    // ---- epilogue: lane (col, q) holds channels nb + 16 f + 4 q .. + 3 of pixel m0 + 16 j + col ----
    const int n0 = nb + 4 * q, n1 = n0 + 16;
    const float4v zf = {0.f, 0.f, 0.f, 0.f};
    const float4v b0 = n0 < a.N ? *reinterpret_cast<const float4v*>(a.bias + n0) : zf;
    const float4v b1 = n1 < a.N ? *reinterpret_cast<const float4v*>(a.bias + n1) : zf;
#pragma unroll
    for (int j = 0; j < MF; ++j) {
      if ((j & wmask) != wm) continue;                    // wave-uniform
      reg_tie(acc[j][0]);
      reg_tie(acc[j][1]);
      const int m = m0 + 16 * j + col;
      const bool mok = m < a.M;
      const size_t rowoff = (size_t)m * a.N;
      float4v v0 = acc[j][0] + b0, v1 = acc[j][1] + b1;
      if constexpr (F16) {
        if (a.res != nullptr && mok) {
          const half_t* rp = static_cast<const half_t*>(a.res) + rowoff;
          if (n0 < a.N) {
            const half4v r = *reinterpret_cast<const half4v*>(rp + n0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v0[e] += a.res_act == 3 ? (float)(half_t)pw_act((float)r[e], 3) : (float)r[e];
          }
          if (n1 < a.N) {
            const half4v r = *reinterpret_cast<const half4v*>(rp + n1);
#pragma unroll
            for (int e = 0; e < 4; ++e) v1[e] += a.res_act == 3 ? (float)(half_t)pw_act((float)r[e], 3) : (float)r[e];
          }
        }
        half4v o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o0[e] = (half_t)pw_act(v0[e], a.act);
          o1[e] = (half_t)pw_act(v1[e], a.act);
        }
        const u32x4_sw sw = split_swap_out(o0, o1);       // every lane swaps
        const int off = f16_pair_off(nb, q);              // 8 consecutive channels
        if (mok && off < a.N) *reinterpret_cast<u32x4_sw*>(static_cast<half_t*>(a.y) + rowoff + off) = sw;
      } else {
        if (a.res != nullptr && mok) {
          const float* rp = static_cast<const float*>(a.res) + rowoff;
          float4v r0 = n0 < a.N ? *reinterpret_cast<const float4v*>(rp + n0) : zf;
          float4v r1 = n1 < a.N ? *reinterpret_cast<const float4v*>(rp + n1) : zf;
          if (a.res_act == 3) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              r0[e] = pw_act(r0[e], 3);
              r1[e] = pw_act(r1[e], 3);
            }
          }
          v0 += r0;
          v1 += r1;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v0[e] = pw_act(v0[e], a.act);
          v1[e] = pw_act(v1[e], a.act);
        }
        float* yp = static_cast<float*>(a.y) + rowoff;
        if (mok && n0 < a.N) *reinterpret_cast<float4v*>(yp + n0) = v0;
        if (mok && n1 < a.N) *reinterpret_cast<float4v*>(yp + n1) = v1;
      }
    }
  }
}

int conv1x1_narrow_kpad(int K, bool f32) {
  const int ks = f32 ? 16 : 32;
  return (K + ks - 1) / ks * ks;
}

template <typename T, int MF, bool SCALE>
static void pw_launch_as(const PwArgs& a, int lds, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&conv1x1_narrow_kernel<T, MF, SCALE>), kPwLdsBytes);
  const int grid = (a.M + 16 * MF - 1) / (16 * MF);
  hipLaunchKernelGGL((conv1x1_narrow_kernel<T, MF, SCALE>), dim3(grid), dim3(256), lds, st, a);
}

template <typename T, int MF>
static void pw_launch(const PwArgs& a, int lds, hipStream_t st) {
  if (a.in_scale != nullptr) pw_launch_as<T, MF, true>(a, lds, st);
  else pw_launch_as<T, MF, false>(a, lds, st);
}

bool conv1x1_narrow_launch(const void* x, int ldx, const void* w, const float* bias, const void* res, void* y, int M,
                           int K, int N, int act, bool f32, hipStream_t st, const void* in_scale, int hw, int res_act) {
  if (M <= 0 || K <= 0 || N <= 0 || K % 8 || N % 8 || K > 1280 || N > 1280 || ldx < K || act < 0 || act > 4)
    return false;
  if ((in_scale != nullptr && (hw <= 0 || M % hw)) || (res_act != 0 && res_act != 3)) return false;
  PwArgs a{};
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.res = res;
  a.y = y;
  a.M = M; a.K = K; a.N = N;
  a.Kp = conv1x1_narrow_kpad(K, f32);
  a.ldx = ldx;
  a.act = act;
  a.in_scale = in_scale;
  a.hw = hw;
  a.res_act = res_act;
  const int pitch = a.Kp * (f32 ? 4 : 2) + 16;
  int mf = 4;
  while (mf > 1 && (16 * mf * pitch > kPwLdsBytes || 16 * (mf / 2) >= M)) mf /= 2;   // fits LDS; no all-idle fragments
  const int lds = 16 * mf * pitch;
  if (lds > kPwLdsBytes) return false;
  const int npairs = (N + 31) / 32, wn = npairs >= 3 ? 4 : npairs;
  a.wm = 4 / wn < mf ? 4 / wn : mf;
  if (f32) {
    if (mf == 4) pw_launch<float, 4>(a, lds, st);
    else if (mf == 2) pw_launch<float, 2>(a, lds, st);
    else pw_launch<float, 1>(a, lds, st);
  } else {
    if (mf == 4) pw_launch<half_t, 4>(a, lds, st);
    else if (mf == 2) pw_launch<half_t, 2>(a, lds, st);
    else pw_launch<half_t, 1>(a, lds, st);
  }
  return true;
}

}  // namespace idunno
