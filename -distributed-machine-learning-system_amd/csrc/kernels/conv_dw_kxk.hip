// Depthwise k x k conv (k = 3 or 5, pad k / 2, stride 1 or 2) + bias (+ReLU / ReLU6 /
// hardswish) on NHWC fp16 or fp32 activations for gfx950, with an optional fused spatial
// mean of its own output: the middle conv of MobileNetV3's blocks and the squeeze of its
// squeeze-and-excitation layers.
//
// Like conv3x3_dw.hip this is a byte mover: 16-byte accesses only, every input row leaves
// HBM once per band, borders are predication, no LDS for the window.  What differs is how
// the window is held.  A rolling k-row x k-column register window would need 25 input
// vectors next to the 25 weight vectors at k = 5, so the walk is transposed:
//
//   * A lane owns one 16-byte channel vector (8 halfs / 4 floats) of one output column and
//     walks INPUT rows downwards.  Input row t of the walk is loaded once, as the lane's k
//     column vectors, and added into every output row it belongs to: output row r takes it
//     with tap row ky = t - S r.  At most NA = k (stride 1) or (k + 1) / 2 (stride 2)
//     output rows are live at a time; their f32 accumulators sit in NA register slots, row
//     r in slot r mod NA.  After input row S r + k - 1 output row r is complete: bias is
//     already in it, the activation is applied, the row is stored and its slot restarts
//     from the bias for row r + NA.  Registers: NA E floats of accumulators, k loaded
//     vectors and the k k weight vectors (tap-major [k k, C]: one 16-byte load a tap).
//   * The walk is unrolled over one period of NA S input rows, so that every slot index and
//     every "does tap row ky hit this input row" test is a compile-time constant and the
//     accumulators never leave registers.  Rows above the first output row of a band are
//     accumulated into slots that restart before their real row begins (k - 1 < NA S).
//   * Products are formed in f32 (a half x half product is exact there) and accumulated in
//     f32; ``act_in`` = 3 applies hardswish to every loaded value, rounded to the
//     activations' dtype: the hardswish of a producer that only has a ReLU epilogue
//     (MobileNetV3's stem runs on the small-C conv kernels without activation).
//
// Two splits of the work over lanes share that walk:
//
//   * plain: conv3x3_dw.hip's.  The flat lane index runs over (image, output column,
//     channel vector), channel vector fastest; bands of 16 output rows (8 at stride 2), the
//     band index fastest in the grid so the k - S halo rows two bands share meet in L2.
//   * pooled (``pool`` output): a workgroup owns ONE image, all its output rows and
//     columns and a group of G <= 256 / Wo channel vectors (lane = column G + vector).  A
//     lane sums the values it stores, as rounded to the output dtype, in f32 registers over
//     the whole column; the Wo column sums of a channel vector then meet in LDS and one
//     lane adds them in column order.  No atomics: the mean is bit-identical from run to
//     run, and the squeeze costs no second pass over the depthwise output.
#include "../common.h"
#include "../kernels.h"

namespace idunno {

struct DwkArgs {
  const void* x;
  const void* w;        // [k k, C] in x's dtype
  const float* bias;    // [C]
  void* y;
  void* pool;           // [B, C] in x's dtype (pooled split) or null
  int B, H, W, C, Ho, Wo;
  int th, nbands;       // plain: output rows per band, bands per image
  int total;            // plain: B * Wo * (C / E) lanes per band
  int G, ngroups;       // pooled: channel vectors per workgroup, workgroups per image
  float inv_hw;         // pooled: 1 / (Ho Wo)
  int act, act_in;
};

template <typename T>
struct DwkVec;
template <>
struct DwkVec<half_t> {
  typedef half8v type;
};
template <>
struct DwkVec<float> {
  typedef float4v type;
};

// Keeps a weight vector in its own registers in its own precision across a walk step: without it the
// compiler converts all k k fp16 weight vectors to f32 ahead of the loop (8 registers a tap instead of 4).
__device__ __forceinline__ void dwk_tie(half8v& r) { asm volatile("" : "+v"(r)); }
__device__ __forceinline__ void dwk_tie(float4v&) {}

__device__ __forceinline__ float dwk_hswish(float v) { return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f); }

// Output rows [oy0, oy1) of output column ox for the lane's channel vector; xb / yb point at the
// vector in pixel (0, 0) of the lane's image.  psum += the stored values (POOL).
template <typename T, int K, int S, bool POOL>
__device__ __forceinline__ void dwk_walk(const DwkArgs& a, const T* xb, T* yb, const T* wp, const float* bp, int ox,
                                         int oy0, int oy1, float* psum) {
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int P = K / 2, NA = S == 1 ? K : (K + 1) / 2, PER = NA * S;
  static_assert(K - 1 < PER, "a slot must restart before its next row begins");
  typedef typename DwkVec<T>::type V;
  const int C = a.C, H = a.H, W = a.W;

  V wv[K * K];
#pragma unroll
  for (int k = 0; k < K * K; ++k) wv[k] = *reinterpret_cast<const V*>(wp + (size_t)k * C);
  float bv[E];
#pragma unroll
  for (int e = 0; e < E; e += 4) {
    const float4v q = *reinterpret_cast<const float4v*>(bp + e);
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[e + i] = q[i];
  }
  float acc[NA][E];
#pragma unroll
  for (int s = 0; s < NA; ++s)
#pragma unroll
    for (int e = 0; e < E; ++e) acc[s][e] = bv[e];

  const int ix0 = ox * S - P;
  bool cok[K];
#pragma unroll
  for (int kx = 0; kx < K; ++kx) cok[kx] = ix0 + kx >= 0 && ix0 + kx < W;
  const int iy0 = oy0 * S - P;                       // input row of walk step 0
  const int tlast = S * (oy1 - oy0 - 1) + K - 1;     // the last output row's last input row
  const bool hsw_in = a.act_in == 3;

  for (int t0 = 0; t0 <= tlast; t0 += PER) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int t = t0 + j, iy = iy0 + t;
      if (t > tlast) continue;                       // workgroup-uniform
      if (iy >= 0 && iy < H) {                       // workgroup-uniform; a row outside adds nothing
        V r[K];
        const T* p = xb + ((long)iy * W + ix0) * C;
#pragma unroll
        for (int k = 0; k < K * K; ++k) dwk_tie(wv[k]);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
#pragma unroll
          for (int e = 0; e < E; ++e) r[kx][e] = (T)0.f;
          if (cok[kx]) r[kx] = *reinterpret_cast<const V*>(p + (long)kx * C);
        }
        if (hsw_in) {
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int e = 0; e < E; ++e) r[kx][e] = (T)dwk_hswish((float)r[kx][e]);
        }
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          if ((j - ky + PER) % S != 0) continue;     // compile time: tap row ky never meets this input row
          const int slot = ((j - ky + PER) / S) % NA;
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[slot][e] = fmaf((float)r[kx][e], (float)wv[ky * K + kx][e], acc[slot][e]);
        }
      }
      if ((j - (K - 1) + PER) % S == 0) {            // compile time: an output row ends with this input row
        const int slot = ((j - (K - 1) + PER) / S) % NA;
        const int rr = t - (K - 1);                  // S * (the row, relative to oy0); negative above the band
        if (rr >= 0) {
          V o;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            float v = acc[slot][e];
            if (a.act == 3) {
              v = dwk_hswish(v);
            } else {
              if (a.act) v = fmaxf(v, 0.f);
              if (a.act == 2) v = fminf(v, 6.f);
            }
            o[e] = (T)v;
            if (POOL) psum[e] += (float)o[e];
          }
          *reinterpret_cast<V*>(yb + ((size_t)(oy0 + rr / S) * a.Wo + ox) * C) = o;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) acc[slot][e] = bv[e];
      }
    }
  }
}

template <typename T, int K, int S>
__global__ void __launch_bounds__(256) conv_dw_kxk_kernel(const DwkArgs a) {
  constexpr int E = 16 / (int)sizeof(T);
  const int blk = blockIdx.x;
  const int band = blk % a.nbands;
  const int idx = (blk / a.nbands) * 256 + (int)threadIdx.x;
  if (idx >= a.total) return;
  const int cvs = a.C / E;
  const int cv = idx % cvs;
  const int t = idx / cvs;
  const int ox = t % a.Wo, b = t / a.Wo;
  const int oy0 = band * a.th, oy1 = min(a.Ho, oy0 + a.th);
  const T* xb = static_cast<const T*>(a.x) + (size_t)b * a.H * a.W * a.C + cv * E;
  T* yb = static_cast<T*>(a.y) + (size_t)b * a.Ho * a.Wo * a.C + cv * E;
  dwk_walk<T, K, S, false>(a, xb, yb, static_cast<const T*>(a.w) + cv * E, a.bias + cv * E, ox, oy0, oy1, nullptr);
}

template <typename T, int K, int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) conv_dw_kxk_pool_kernel(const DwkArgs a) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename DwkVec<T>::type V;
  __shared__ float part[256 * E];                    // [column][vector of the group][E]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.ngroups, grp = blockIdx.x % a.ngroups;
  const int cvs = a.C / E;
  const int g = tid % a.G, ox = tid / a.G;
  const int cv = grp * a.G + g;
  float psum[E];
#pragma unroll
  for (int e = 0; e < E; ++e) psum[e] = 0.f;
  const bool live = ox < a.Wo && cv < cvs;
  if (live) {
    const T* xb = static_cast<const T*>(a.x) + (size_t)b * a.H * a.W * a.C + cv * E;
    T* yb = static_cast<T*>(a.y) + (size_t)b * a.Ho * a.Wo * a.C + cv * E;
    dwk_walk<T, K, S, true>(a, xb, yb, static_cast<const T*>(a.w) + cv * E, a.bias + cv * E, ox, 0, a.Ho, psum);
  }
  if (ox < a.Wo) {
#pragma unroll
    for (int e = 0; e < E; ++e) part[tid * E + e] = psum[e];
  }
  __syncthreads();
  if (tid < a.G && cv < cvs) {                       // tid = g: column 0's lanes add the columns in order
    V m;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float s = 0.f;
      for (int c = 0; c < a.Wo; ++c) s += part[(c * a.G + tid) * E + e];
      m[e] = (T)(s * a.inv_hw);
    }
    *reinterpret_cast<V*>(static_cast<T*>(a.pool) + (size_t)b * a.C + cv * E) = m;
  }
}

bool conv_dw_pool_ok(int Wo) { return Wo >= 1 && Wo <= 256; }

template <typename T, int K>
static void dwk_launch(const DwkArgs& a, int stride, dim3 g, hipStream_t st) {
  if (a.pool != nullptr) {
    if (stride == 1) hipLaunchKernelGGL((conv_dw_kxk_pool_kernel<T, K, 1>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_dw_kxk_pool_kernel<T, K, 2>), g, dim3(256), 0, st, a);
  } else {
    if (stride == 1) hipLaunchKernelGGL((conv_dw_kxk_kernel<T, K, 1>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_dw_kxk_kernel<T, K, 2>), g, dim3(256), 0, st, a);
  }
}

bool conv_dw_kxk_launch(const void* x, const void* w, const float* bias, void* y, void* pool, int B, int H, int W, int C,
                        int k, int stride, int act, int act_in, bool f32, hipStream_t st) {
  const int E = f32 ? 4 : 8;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % E || (k != 3 && k != 5) || (stride != 1 && stride != 2) || act < 0 ||
      act > 3 || (act_in != 0 && act_in != 3))
    return false;
  DwkArgs a{};
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.y = y;
  a.pool = pool;
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.Ho = (H - 1) / stride + 1;
  a.Wo = (W - 1) / stride + 1;
  a.act = act;
  a.act_in = act_in;
  const int cvs = C / E;
  long grid;
  if (pool != nullptr) {
    if (!conv_dw_pool_ok(a.Wo)) return false;
    const int gmax = 256 / a.Wo < cvs ? 256 / a.Wo : cvs;
    a.ngroups = (cvs + gmax - 1) / gmax;
    a.G = (cvs + a.ngroups - 1) / a.ngroups;         // even groups: Wo * G <= 256 lanes
    a.inv_hw = 1.f / ((float)a.Ho * (float)a.Wo);
    a.nbands = 1;
    a.th = a.Ho;
    grid = (long)B * a.ngroups;
  } else {
    const int rows = stride == 1 ? 16 : 8;
    a.nbands = (a.Ho + rows - 1) / rows;
    a.th = (a.Ho + a.nbands - 1) / a.nbands;
    const long total = (long)B * a.Wo * cvs;
    if (total >= (1L << 31)) return false;
    a.total = (int)total;
    grid = (total + 255) / 256 * a.nbands;
  }
  if (grid >= (1L << 31)) return false;
  const dim3 g((unsigned)grid);
  if (f32) {
    if (k == 3) dwk_launch<float, 3>(a, stride, g, st);
    else dwk_launch<float, 5>(a, stride, g, st);
  } else {
    if (k == 3) dwk_launch<half_t, 3>(a, stride, g, st);
    else dwk_launch<half_t, 5>(a, stride, g, st);
  }
  return true;
}

}  // namespace idunno
