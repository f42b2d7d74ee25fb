// Squeeze-and-excitation gate in one launch, fp16 or fp32, for gfx950:
//
//   scale[B, C] = hardsigmoid(W2 relu(W1 mean + b1) + b2),   W1 [Csq, C], W2 [C, Csq]
//
// (MobileNetV3's SE layers; C <= 1280, Csq <= 320, both multiples of 8).  Both GEMMs have
// M = B, a few hundred rows at most, and sit on the critical path of every SE block between
// the depthwise conv that produces ``mean`` and the project conv that consumes ``scale``:
// the work is tiny, the cost is launches and round trips through memory, so the hidden
// vector never leaves the CU.
//
//   * A workgroup (4 waves) owns 16 images: one MFMA pixel fragment.  Their mean rows are
//     staged once into padded LDS with 16-byte accesses, zero-filled from C up to the K
//     step and for the rows past B, exactly like conv1x1_narrow.hip's tile (the weights'
//     zero pad never multiplies stale LDS contents).
//   * FC1 runs on v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x4_f32 with the weights
//     (pack_pw_weight: [N, Kp], zero from K) as the A operand and the images as the B
//     operand, so a lane ends with four consecutive hidden channels of one image.  The
//     waves share the 32-channel fragment pairs; a pair's weight fragments of the next K
//     step are fetched from L2 under this step's MFMAs.
//   * bias + ReLU, then the hidden [16, Csq] goes back to a second padded LDS tile in the
//     activations' dtype (what the reference module's fc1 output is rounded to), written
//     as zeros from Csq up to FC2's K step: channels past Csq have zero weights and a
//     predicated-off bias, so the same code path produces them.
//   * One barrier, then FC2 reads that tile as its B operand, adds bias, applies
//     hardsigmoid and stores ``scale``: fp32 as float4s, fp16 after trading halves between
//     the pair's fragments (v_permlane16_swap) as one 16-byte store a lane.  Images past B
//     and channel chunks past C are predicated off.
//   * LDS rows are padded by 16 bytes (an odd number of 16-byte slots a row): the 16 lanes
//     of a ds_read_b128 lane group, 16 images at one k chunk, fall on different banks.
#include "../common.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

struct SeArgs {
  const void* mean;     // [B, C] in the activations' dtype
  const void* w1;       // [Csq, Kp1], zero from C
  const float* b1;      // [Csq]
  const void* w2;       // [C, Kp2], zero from Csq
  const float* b2;      // [C]
  void* scale;          // [B, C]
  int B, C, Csq, Kp1, Kp2;
};

constexpr int kSeLdsBytes = 16 * (1280 * 4 + 16) + 16 * (320 * 4 + 16);   // widest fp32 tiles: 100.5 KiB

template <typename T>
struct SeFrag;
template <>
struct SeFrag<half_t> {
  typedef half8v type;
  static __device__ __forceinline__ float4v mma(half8v a, half8v b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct SeFrag<float> {
  typedef float4v type;
  static __device__ __forceinline__ float4v mma(float4v a, float4v b, float4v c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], c, 0, 0, 0);
    return c;
  }
};

// acc0 / acc1 = the 16-channel fragments nb .. nb + 15 / nb + 16 .. nb + 31 of w[N, Kp] times the 16 LDS
// rows at ``rows``: lane (col, q) ends with channels nb (+ 16) + 4 q .. + 3 of row col.
template <typename T>
__device__ __forceinline__ void se_pair(const char* rows, int pitch, const T* w, int Kp, int N, int nb, int col, int q,
                                        float4v& acc0, float4v& acc1) {
  constexpr int E = 16 / (int)sizeof(T), KS = 4 * E;
  typedef typename SeFrag<T>::type V;
  const bool ok0 = nb + col < N, ok1 = nb + 16 + col < N;
  const T* w0 = w + (size_t)(nb + col) * Kp + q * E;
  const T* w1 = w0 + (size_t)16 * Kp;
  const char* brow = rows + col * pitch + q * 16;
  V zero;
#pragma unroll
  for (int e = 0; e < E; ++e) zero[e] = (T)0.f;
  acc0 = acc1 = float4v{0.f, 0.f, 0.f, 0.f};
  const int nks = Kp / KS;
  V a0n = ok0 ? *reinterpret_cast<const V*>(w0) : zero;
  V a1n = ok1 ? *reinterpret_cast<const V*>(w1) : zero;
  for (int ks = 0; ks < nks; ++ks) {
    const V a0 = a0n, a1 = a1n;
    if (ks + 1 < nks) {
      a0n = ok0 ? *reinterpret_cast<const V*>(w0 + (ks + 1) * KS) : zero;
      a1n = ok1 ? *reinterpret_cast<const V*>(w1 + (ks + 1) * KS) : zero;
    }
    const V bx = *reinterpret_cast<const V*>(brow + ks * (KS * (int)sizeof(T)));
    acc0 = SeFrag<T>::mma(a0, bx, acc0);
    acc1 = SeFrag<T>::mma(a1, bx, acc1);
  }
  reg_tie(acc0);
  reg_tie(acc1);
}

template <typename T>
__global__ void __launch_bounds__(256) se_excite_kernel(const SeArgs a) {
  constexpr int E = 16 / (int)sizeof(T);
  constexpr bool F16 = sizeof(T) == 2;
  typedef typename SeFrag<T>::type V;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int b0 = blockIdx.x * 16;
  const int pitch1 = a.Kp1 * (int)sizeof(T) + 16, pitch2 = a.Kp2 * (int)sizeof(T) + 16;   // bytes
  char* hid = smem + 16 * pitch1;

  // ---- stage the 16 mean rows: 16 bytes a lane, zeros past C and past B ---------------------------
  {
    const int cpr = a.Kp1 / E, kvc = a.C / E, total = 16 * cpr;
    const T* mb = static_cast<const T*>(a.mean);
    for (int i = tid; i < total; i += 256) {
      const int m = i / cpr, c = i - m * cpr;
      V v;
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = (T)0.f;
      if (b0 + m < a.B && c < kvc) v = *reinterpret_cast<const V*>(mb + (size_t)(b0 + m) * a.C + c * E);
      *reinterpret_cast<V*>(smem + m * pitch1 + c * 16) = v;
    }
  }
  __syncthreads();

  const float4v zf = {0.f, 0.f, 0.f, 0.f};
  // ---- FC1 + bias + ReLU -> hidden tile, zeros from Csq to Kp2 ------------------------------------
  for (int pair = wave; pair * 32 < a.Kp2; pair += 4) {   // wave-uniform
    const int nb = pair * 32;
    float4v acc0, acc1;
    se_pair<T>(smem, pitch1, static_cast<const T*>(a.w1), a.Kp1, a.Csq, nb, col, q, acc0, acc1);
    const int n0 = nb + 4 * q, n1 = n0 + 16;
    const float4v v0 = acc0 + (n0 < a.Csq ? *reinterpret_cast<const float4v*>(a.b1 + n0) : zf);
    const float4v v1 = acc1 + (n1 < a.Csq ? *reinterpret_cast<const float4v*>(a.b1 + n1) : zf);
    T* hrow = reinterpret_cast<T*>(hid + col * pitch2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (n0 < a.Kp2) hrow[n0 + e] = (T)fmaxf(v0[e], 0.f);
      if (n1 < a.Kp2) hrow[n1 + e] = (T)fmaxf(v1[e], 0.f);
    }
  }
  __syncthreads();

  // ---- FC2 + bias + hardsigmoid -> scale ----------------------------------------------------------
  const bool mok = b0 + col < a.B;
  const size_t rowoff = (size_t)(b0 + col) * a.C;
  for (int pair = wave; pair * 32 < a.C; pair += 4) {     // wave-uniform
    const int nb = pair * 32;
    float4v acc0, acc1;
    se_pair<T>(hid, pitch2, static_cast<const T*>(a.w2), a.Kp2, a.C, nb, col, q, acc0, acc1);
    const int n0 = nb + 4 * q, n1 = n0 + 16;
    float4v v0 = acc0 + (n0 < a.C ? *reinterpret_cast<const float4v*>(a.b2 + n0) : zf);
    float4v v1 = acc1 + (n1 < a.C ? *reinterpret_cast<const float4v*>(a.b2 + n1) : zf);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[e] = fminf(fmaxf(v0[e] + 3.f, 0.f), 6.f) * (1.f / 6.f);
      v1[e] = fminf(fmaxf(v1[e] + 3.f, 0.f), 6.f) * (1.f / 6.f);
    }
    if constexpr (F16) {
      half4v o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o0[e] = (half_t)v0[e];
        o1[e] = (half_t)v1[e];
      }
      const u32x4_sw sw = split_swap_out(o0, o1);         // every lane swaps
      const int off = f16_pair_off(nb, q);                // 8 consecutive channels
      if (mok && off < a.C) *reinterpret_cast<u32x4_sw*>(static_cast<half_t*>(a.scale) + rowoff + off) = sw;
    } else {
      float* sp = static_cast<float*>(a.scale) + rowoff;
      if (mok && n0 < a.C) *reinterpret_cast<float4v*>(sp + n0) = v0;
      if (mok && n1 < a.C) *reinterpret_cast<float4v*>(sp + n1) = v1;
    }
  }
}

bool se_excite_launch(const void* mean, const void* w1, const float* b1, const void* w2, const float* b2, void* scale,
                      int B, int C, int Csq, bool f32, hipStream_t st) {
  if (B <= 0 || C <= 0 || Csq <= 0 || C % 8 || Csq % 8 || C > 1280 || Csq > 320) return false;
  SeArgs a{};
  a.mean = mean;
  a.w1 = w1;
  a.b1 = b1;
  a.w2 = w2;
  a.b2 = b2;
  a.scale = scale;
  a.B = B; a.C = C; a.Csq = Csq;
  a.Kp1 = conv1x1_narrow_kpad(C, f32);
  a.Kp2 = conv1x1_narrow_kpad(Csq, f32);
  const int es = f32 ? 4 : 2;
  const int lds = 16 * (a.Kp1 * es + 16) + 16 * (a.Kp2 * es + 16);
  if (lds > kSeLdsBytes) return false;
  const dim3 g((unsigned)((B + 15) / 16));
  if (f32) {
    ensure_lds_attr(reinterpret_cast<const void*>(&se_excite_kernel<float>), kSeLdsBytes);
    hipLaunchKernelGGL((se_excite_kernel<float>), g, dim3(256), lds, st, a);
  } else {
    ensure_lds_attr(reinterpret_cast<const void*>(&se_excite_kernel<half_t>), kSeLdsBytes);
    hipLaunchKernelGGL((se_excite_kernel<half_t>), g, dim3(256), lds, st, a);
  }
  return true;
}

}  // namespace idunno
