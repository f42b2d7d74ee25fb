// DenseNet for gfx950: a dense layer in one launch on the block's concat buffer, the transition (norm + ReLU +
// 2x2 average pool + 1x1 conv) in one launch, and the two small kernels around them.  NHWC fp16 or true fp32 by
// template; bottleneck width M = 128 and growth G = 32 are compile-time constants (dense_math.h).
//
//   t = relu(W1' relu(x s1 + t1) + b1)        x = buf[..., 0:cin],  W1' = conv1 with norm2 folded in, b1 its shift
//   buf[..., cin:cin + 32] = W2 (*)3x3,pad1 t                       no bias, no activation: the next layer's norm1
//
// dense_layer_kernel<T>: a workgroup (4 waves) owns one image and a band of R rows.
//
//   * In place without a race.  Every workgroup of a launch reads channels [0, cin) only -- of its halo rows too --
//     and writes channels [cin, cin + 32) only, so no workgroup reads what another writes: one launch has no
//     inter-workgroup hazard and the concat needs no copy.
//   * Phase 1, the bottleneck.  The band's rows plus one halo row each side, clipped to the image, are one
//     contiguous pixel range (rows are full width) at pixel pitch Ctot.  It is walked in chunks of 16 mf pixels and,
//     inside a pixel chunk, cin is walked in K chunks of kc channels.  The staging pass is the prologue:
//     16-byte loads into registers one chunk AHEAD (issued before the MFMAs of the chunk in LDS, retired after
//     them), then relu(x s1 + t1) in fp32 with s1, t1 read from LDS, one rounding to T, 16-byte LDS stores.
//     Slots without data -- pixels past the range, channels from cin -- are stored as ZERO, never relu(t1).
//     W1' is the A operand: all K steps of the chunk (<= 8, two 16-channel fragments a wave) are loaded before the
//     chunk is staged, so their L2 latency hides behind the prologue and the barrier.  A wave keeps 2 x mf
//     accumulators (its 32 bottleneck channels x the pixel chunk) across the K chunks: 8 mf fragments a workgroup.
//     relu(acc + b1), rounded to T, goes to the bottleneck map in LDS: (R + 2) x (W + 2) pixels of
//     128 sizeof(T) + 16 bytes = 17 / 33 sixteen-byte slots, odd, so the 16 pixel lanes of a ds_read_b128 fall on
//     16 different slots (fire.hip's reasoning).  The map is cleared first and only in-image pixels are written:
//     the 3x3's zero padding applies to the map (a halo computed from zero-padded x would be relu(b1)), and the
//     map never reaches HBM.
//   * Phase 2, the 3x3.  One implicit GEMM over K = 9 x 128 from the map only, tap-major: lane (col, q) of K step
//     ks reads chunk g = 4 ks + q, tap g / CPT at ((dy (W + 2) + dx) pitch + 16 (g % CPT)) past its pixel's window
//     origin.  The 32 outputs are two 16-channel fragments; waves split over pixel fragments, four a wave a pass
//     (fragment f0 + 4 j + wave).  W2 streams from L2 in groups of four K steps, the next group loaded under this
//     group's MFMAs.
//   * Epilogue: the transposed accumulator (a lane: 4 channels of each fragment of one pixel) is stored at
//     buf + pixel Ctot + cin: fp32 two float4s, fp16 one 16-byte store after split_swap_out.
//   * dense_math.h plans R, mf, kc and the LDS bytes; docs/KERNELS.md lists every served layer shape.
//
// dense_transition_kernel<T>: out[..., 0:C/2] = W avgpool2x2(relu(x s + t)).  The pool commutes with the bias-free
// conv, so it runs first: a quarter of the MACs.  Phase 1's machinery with a pooling staging pass (four 16-byte
// loads a slot, prologue on each, the mean in fp32, one rounding); a workgroup owns an image and 128 output
// channels, walks the image's pooled pixels in chunks of 16 mf, and stores like phase 2.
//
// maxpool_into_kernel<T>: a max pool that writes channels [0, C) of a wider buffer (the stem's pool lands in block
// 1's buffer).  bn_relu_avgpool_kernel<T>: mean over pixels of relu(x s + t), fp32 sums in pixel order: the same
// bits every run.
#include "../common.h"
#include "../dense_math.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

using dense::kG;
using dense::kM;

template <typename T>
struct DenseFrag;
template <>
struct DenseFrag<half_t> {
  typedef half8v type;
  typedef half4v out4;
  static __device__ __forceinline__ float4v mma(half8v a, half8v b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct DenseFrag<float> {
  typedef float4v type;
  typedef float4v out4;
  static __device__ __forceinline__ float4v mma(float4v a, float4v b, float4v c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], c, 0, 0, 0);
    return c;
  }
};

template <typename V, typename T>
__device__ __forceinline__ V dense_zero() {
  V z;
#pragma unroll
  for (int e = 0; e < 16 / (int)sizeof(T); ++e) z[e] = (T)0.f;
  return z;
}

// ---- the 1x1 GEMM both big kernels share: 128 output channels x a pixel range, K chunked through LDS -------------
struct DenseSrc {
  const void* base;    // first pixel of the range (POOL: of the image)
  int ld;              // elements from one pixel to the next
  int npix;            // pixels of the range (POOL: pooled pixels of the image)
  int K;               // channels with data
  int W, Wo;           // POOL: source and pooled width
};

template <typename T, bool POOL>
struct DenseStage {
  static constexpr int SZ = (int)sizeof(T), E = 16 / SZ;
  static constexpr int NV = POOL ? 4 : 1;     // 16-byte loads a slot
  static constexpr int NI = POOL ? 4 : 8;     // slots a thread: 16 mf rows x <= 32 chunks over 256 threads
  typedef typename DenseFrag<T>::type V;
  V raw[NI][NV];

  // slot i of the chunk at (m0, k0): row m, 16-byte chunk c; whether it carries data
  static __device__ __forceinline__ bool slot(const DenseSrc& s, int i, int cpr, int m0, int k0, int total, int& m,
                                              int& c) {
    m = i / cpr;
    c = i - m * cpr;
    return i < total && m0 + m < s.npix && k0 + c * E < s.K;
  }

  __device__ __forceinline__ void fetch(const DenseSrc& s, int m0, int k0, int kc, int rows, int tid) {
    const int cpr = kc / E, total = rows * cpr;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      int m, c;
      if (!slot(s, tid + 256 * j, cpr, m0, k0, total, m, c)) continue;
      const int p = m0 + m;
      if constexpr (POOL) {
        const int pr = p / s.Wo, pc = p - pr * s.Wo;
        const T* src = static_cast<const T*>(s.base) + ((size_t)(2 * pr) * s.W + 2 * pc) * s.ld + k0 + c * E;
        raw[j][0] = *reinterpret_cast<const V*>(src);
        raw[j][1] = *reinterpret_cast<const V*>(src + s.ld);
        raw[j][2] = *reinterpret_cast<const V*>(src + (size_t)s.W * s.ld);
        raw[j][3] = *reinterpret_cast<const V*>(src + (size_t)(s.W + 1) * s.ld);
      } else {
        raw[j][0] = *reinterpret_cast<const V*>(static_cast<const T*>(s.base) + (size_t)p * s.ld + k0 + c * E);
      }
    }
  }

  // relu(x scale + shift) (POOL: the mean of four) -> xs; ss = scale [K] then shift [K] floats in LDS
  __device__ __forceinline__ void store(char* xs, const float* ss, const DenseSrc& s, int m0, int k0, int kc, int rows,
                                        int pitch, int tid) const {
    const int cpr = kc / E, total = rows * cpr;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int i = tid + 256 * j;
      if (i >= total) continue;
      int m, c;
      V v = dense_zero<V, T>();
      if (slot(s, i, cpr, m0, k0, total, m, c)) {
        const float* sc = ss + k0 + c * E;
        const float* sh = sc + s.K;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          float f = fmaxf((float)raw[j][0][e] * sc[e] + sh[e], 0.f);
          if constexpr (POOL) {
#pragma unroll
            for (int t = 1; t < 4; ++t) f += fmaxf((float)raw[j][t][e] * sc[e] + sh[e], 0.f);
            f *= 0.25f;
          }
          v[e] = (T)f;
        }
      }
      *reinterpret_cast<V*>(xs + m * pitch + c * 16) = v;
    }
  }
};

struct DenseGemm {
  const void* w;       // [N, Kp] A operand, rows nb + col and nb + 16 + col are this lane's
  int Kp, N, nb;
  int kc, mf;
};

// epi(m0, j, acc0, acc1): lane (col, q) holds channels nb + 4 q .. + 3 (acc0) and nb + 16 + 4 q .. (acc1) of pixel
// m0 + 16 j + col.  Ends on a barrier-free note: the caller syncs before it reads what epi wrote to LDS.
template <typename T, bool POOL, typename Epi>
__device__ __forceinline__ void dense_gemm128(char* xs, const float* ss, const DenseSrc& src, const DenseGemm& g, int tid,
                                              Epi epi) {
  constexpr int SZ = (int)sizeof(T), E = 16 / SZ, KS = 4 * E, MAXKS = dense::kMaxChunkBytes / dense::kStepBytes;
  typedef typename DenseFrag<T>::type V;
  const int lane = tid & 63, col = lane & 15, q = lane >> 4;
  const int pitch = g.kc * SZ + 16, rows = 16 * g.mf;
  const int nkc = (g.Kp + g.kc - 1) / g.kc, nmc = (src.npix + rows - 1) / rows, nit = nkc * nmc;
  const bool ok0 = g.nb + col < g.N, ok1 = g.nb + 16 + col < g.N;
  const T* w0 = static_cast<const T*>(g.w) + (size_t)(g.nb + col) * g.Kp + q * E;
  const T* w1 = w0 + (size_t)16 * g.Kp;
  const char* brow = xs + col * pitch + q * 16;
  const V zero = dense_zero<V, T>();
  const float4v zf = {0.f, 0.f, 0.f, 0.f};

  DenseStage<T, POOL> st;
  float4v acc[2][4];
  st.fetch(src, 0, 0, min(g.kc, g.Kp), rows, tid);
  for (int it = 0; it < nit; ++it) {
    const int mc = it / nkc, kci = it - mc * nkc;
    const int m0 = mc * rows, k0 = kci * g.kc, kc = min(g.kc, g.Kp - k0), nks = kc / KS;
    if (kci == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[0][j] = acc[1][j] = zf;
    }
    V wr[MAXKS][2];                                           // this chunk's weights: in flight under the prologue
#pragma unroll
    for (int ks = 0; ks < MAXKS; ++ks) {
      wr[ks][0] = wr[ks][1] = zero;
      if (ks < nks) {                                         // wave-uniform
        if (ok0) wr[ks][0] = *reinterpret_cast<const V*>(w0 + k0 + ks * KS);
        if (ok1) wr[ks][1] = *reinterpret_cast<const V*>(w1 + k0 + ks * KS);
      }
    }
    st.store(xs, ss, src, m0, k0, kc, rows, pitch, tid);
    __syncthreads();
    if (it + 1 < nit) {                                       // the next chunk's loads fly under these MFMAs
      const int mc2 = (it + 1) / nkc, k2 = (it + 1 - mc2 * nkc) * g.kc;
      st.fetch(src, mc2 * rows, k2, min(g.kc, g.Kp - k2), rows, tid);
    }
#pragma unroll
    for (int ks = 0; ks < MAXKS; ++ks) {
      if (ks >= nks) continue;                                // wave-uniform
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= g.mf) continue;                              // wave-uniform
        const V bx = *reinterpret_cast<const V*>(brow + 16 * j * pitch + ks * dense::kStepBytes);
        acc[0][j] = DenseFrag<T>::mma(wr[ks][0], bx, acc[0][j]);
        acc[1][j] = DenseFrag<T>::mma(wr[ks][1], bx, acc[1][j]);
      }
    }
    __syncthreads();                                          // the chunk is read: the next store may overwrite it
    if (kci == nkc - 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < g.mf) epi(m0, j, acc[0][j], acc[1][j]);
    }
  }
}

// scale [K] and shift [K] -> LDS
__device__ __forceinline__ void dense_stage_norm(float* ss, const float* scale, const float* shift, int K, int tid) {
  for (int i = tid * 4; i < K; i += 256 * 4) {
    *reinterpret_cast<float4v*>(ss + i) = *reinterpret_cast<const float4v*>(scale + i);
    *reinterpret_cast<float4v*>(ss + K + i) = *reinterpret_cast<const float4v*>(shift + i);
  }
}

// a pixel's 32 channels from the two transposed fragments: lane (col, q) holds channels 4 q .. + 3 of each
template <typename T>
__device__ __forceinline__ void dense_store_pair(T* row, int nb, int lim, int q, bool mok, float4v v0, float4v v1) {
  if constexpr (sizeof(T) == 2) {
    half4v o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = (half_t)v0[e];
      o1[e] = (half_t)v1[e];
    }
    const u32x4_sw sw = split_swap_out(o0, o1);               // every lane swaps
    const int off = f16_pair_off(nb, q);                      // 8 consecutive channels
    if (mok && off < lim) *reinterpret_cast<u32x4_sw*>(row + off) = sw;
  } else {
    const int n0 = nb + 4 * q, n1 = n0 + 16;
    if (mok && n0 < lim) *reinterpret_cast<float4v*>(row + n0) = v0;
    if (mok && n1 < lim) *reinterpret_cast<float4v*>(row + n1) = v1;
  }
}

// ---- the dense layer ---------------------------------------------------------------------------------------------
struct DenseLayerArgs {
  void* buf;            // [B, H, W, Ctot]: reads channels [0, cin), writes [cin, cin + 32)
  const float* scale1;  // [cin]
  const float* shift1;  // [cin]
  const void* w1;       // [128, cin]
  const float* b1;      // [128]
  const void* w2;       // [32, 9 * 128] tap-major
  int B, H, W, cin, Ctot;
  int R, nbands, mf, kc, xbytes, ssbytes;
};

constexpr int kDenseMP = 4;     // pixel fragments a wave a pass of the 3x3
constexpr int kDenseGK = 4;     // K steps a weight group of the 3x3

template <typename T>
__global__ void __launch_bounds__(256) dense_layer_kernel(const DenseLayerArgs a) {
  constexpr int SZ = (int)sizeof(T), E = 16 / SZ, KS = 4 * E, CPT = kM / E, PM = dense::map_pitch(SZ);
  constexpr int NKS = 9 * kM / KS, NGR = NKS / kDenseGK;
  static_assert(NKS % kDenseGK == 0, "the 3x3's K steps come in whole groups");
  typedef typename DenseFrag<T>::type V;
  typedef typename DenseFrag<T>::out4 O4;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / a.nbands, band = blockIdx.x - b * a.nbands;
  const int r0 = band * a.R, rows = min(a.R, a.H - r0);
  const int W2 = a.W + 2;
  float* ss = reinterpret_cast<float*>(smem + a.xbytes);
  char* map = smem + a.xbytes + a.ssbytes;                    // [rows + 2][W + 2][PM]
  const V zero = dense_zero<V, T>();
  const float4v zf = {0.f, 0.f, 0.f, 0.f};
  T* img = static_cast<T*>(a.buf) + (size_t)b * a.H * a.W * a.Ctot;

  for (int i = tid * 16; i < (rows + 2) * W2 * PM; i += 256 * 16) *reinterpret_cast<V*>(map + i) = zero;
  dense_stage_norm(ss, a.scale1, a.shift1, a.cin, tid);
  __syncthreads();

  // ---- phase 1: image rows [rlo, rhi) -> map rows rlo - (r0 - 1) ... ------------------------------------------
  {
    const int rlo = max(r0 - 1, 0), rhi = min(r0 + rows + 1, a.H);
    DenseSrc src{img + (size_t)rlo * a.W * a.Ctot, a.Ctot, (rhi - rlo) * a.W, a.cin, 0, 0};
    DenseGemm g{a.w1, a.cin, kM, wave * 32, a.kc, a.mf};
    const float4v bq0 = *reinterpret_cast<const float4v*>(a.b1 + g.nb + 4 * q);
    const float4v bq1 = *reinterpret_cast<const float4v*>(a.b1 + g.nb + 16 + 4 * q);
    char* mrow = map + ((rlo - (r0 - 1)) * W2 + 1) * PM + (g.nb + 4 * q) * SZ;
    dense_gemm128<T, false>(smem, ss, src, g, tid, [&](int m0, int j, float4v c0, float4v c1) {
      const int m = m0 + 16 * j + col;
      if (m >= src.npix) return;
      const int pr = m / a.W, pc = m - pr * a.W;
      O4 o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o0[e] = (T)fmaxf(c0[e] + bq0[e], 0.f);
        o1[e] = (T)fmaxf(c1[e] + bq1[e], 0.f);
      }
      char* dst = mrow + (pr * W2 + pc) * PM;
      *reinterpret_cast<O4*>(dst) = o0;
      *reinterpret_cast<O4*>(dst + 16 * SZ) = o1;
    });
  }
  __syncthreads();

  // ---- phase 2: the 3x3 over the map ------------------------------------------------------------------------------
  const int npo = rows * a.W, nfrag = (npo + 15) / 16;
  const T* w0 = static_cast<const T*>(a.w2) + (size_t)col * (9 * kM) + q * E;
  const T* w1 = w0 + (size_t)16 * (9 * kM);
  T* orow = img + (size_t)r0 * a.W * a.Ctot + a.cin;          // the band's first output pixel, channel cin

  for (int f0 = 0; f0 < nfrag; f0 += 4 * kDenseMP) {
    if (f0 + wave >= nfrag) break;                            // wave-uniform: no fragment of this pass is this wave's
    int base[kDenseMP];                                       // window origin of this lane's pixel of fragment f0 + 4 j + wave
    float4v acc[kDenseMP][2];
#pragma unroll
    for (int j = 0; j < kDenseMP; ++j) {
      const int p = (f0 + 4 * j + wave) * 16 + col, pp = p < npo ? p : 0;
      const int r = pp / a.W, c = pp - r * a.W;
      base[j] = (r * W2 + c) * PM;
      acc[j][0] = acc[j][1] = zf;
    }
    V cur[kDenseGK][2], nxt[kDenseGK][2];
#pragma unroll
    for (int s = 0; s < kDenseGK; ++s) {
      nxt[s][0] = *reinterpret_cast<const V*>(w0 + s * KS);
      nxt[s][1] = *reinterpret_cast<const V*>(w1 + s * KS);
    }
    for (int gr = 0; gr < NGR; ++gr) {
#pragma unroll
      for (int s = 0; s < kDenseGK; ++s) {
        cur[s][0] = nxt[s][0];
        cur[s][1] = nxt[s][1];
      }
      if (gr + 1 < NGR) {
#pragma unroll
        for (int s = 0; s < kDenseGK; ++s) {
          nxt[s][0] = *reinterpret_cast<const V*>(w0 + ((gr + 1) * kDenseGK + s) * KS);
          nxt[s][1] = *reinterpret_cast<const V*>(w1 + ((gr + 1) * kDenseGK + s) * KS);
        }
      }
#pragma unroll
      for (int s = 0; s < kDenseGK; ++s) {
        const int gch = (gr * kDenseGK + s) * 4 + q, tap = gch / CPT, cc = gch - tap * CPT;
        const int dy = tap / 3, dx = tap - 3 * dy;
        const int off = (dy * W2 + dx) * PM + cc * 16;
#pragma unroll
        for (int j = 0; j < kDenseMP; ++j) {
          if (f0 + 4 * j + wave >= nfrag) continue;           // wave-uniform
          const V bx = *reinterpret_cast<const V*>(map + base[j] + off);
          acc[j][0] = DenseFrag<T>::mma(cur[s][0], bx, acc[j][0]);
          acc[j][1] = DenseFrag<T>::mma(cur[s][1], bx, acc[j][1]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kDenseMP; ++j) {
      if (f0 + 4 * j + wave >= nfrag) continue;               // wave-uniform
      reg_tie(acc[j][0]);
      reg_tie(acc[j][1]);
      const int p = (f0 + 4 * j + wave) * 16 + col;
      dense_store_pair<T>(orow + (size_t)p * a.Ctot, 0, kG, q, p < npo, acc[j][0], acc[j][1]);
    }
  }
}

bool dense_layer_ok(int H, int W, int cin, int Ctot, bool f32) {
  dense::Plan p;
  return Ctot > 0 && Ctot % 8 == 0 && cin + kG <= Ctot && dense::plan(H, W, cin, f32, p);
}

bool dense_plan(int H, int W, int cin, bool f32, int out[6]) {
  dense::Plan p;
  if (!dense::plan(H, W, cin, f32, p)) return false;
  out[0] = p.R; out[1] = p.nbands; out[2] = p.mf; out[3] = p.kc; out[4] = p.xbytes; out[5] = p.lds;
  return true;
}

template <typename T>
static void dense_layer_launch_as(const DenseLayerArgs& a, int lds, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&dense_layer_kernel<T>), dense::kBudget);
  hipLaunchKernelGGL((dense_layer_kernel<T>), dim3((unsigned)(a.B * a.nbands)), dim3(256), lds, st, a);
}

bool dense_layer_launch(void* buf, const float* scale1, const float* shift1, const void* w1, const float* b1,
                        const void* w2, int B, int H, int W, int cin, int Ctot, bool f32, hipStream_t st) {
  dense::Plan p;
  if (B <= 0 || !dense_layer_ok(H, W, cin, Ctot, f32) || !dense::plan(H, W, cin, f32, p)) return false;
  if ((long)B * p.nbands >= (1L << 31)) return false;
  DenseLayerArgs a{};
  a.buf = buf; a.scale1 = scale1; a.shift1 = shift1; a.w1 = w1; a.b1 = b1; a.w2 = w2;
  a.B = B; a.H = H; a.W = W; a.cin = cin; a.Ctot = Ctot;
  a.R = p.R; a.nbands = p.nbands; a.mf = p.mf; a.kc = p.kc; a.xbytes = p.xbytes; a.ssbytes = p.ssbytes;
  if (f32) dense_layer_launch_as<float>(a, p.lds, st);
  else dense_layer_launch_as<half_t>(a, p.lds, st);
  return true;
}

// ---- the transition ----------------------------------------------------------------------------------------------
struct DenseTransArgs {
  const void* x;        // [B, H, W, C]
  const float* scale;   // [C]
  const float* shift;   // [C]
  const void* w;        // [C / 2, C]
  void* out;            // [B, H / 2, W / 2, ldo]: channels [0, C / 2) are written
  int H, W, C, N, Ho, Wo, ldo;
  int nsl;              // 128-channel slices of N
  int mf, kc, xbytes;
};

template <typename T>
__global__ void __launch_bounds__(256) dense_transition_kernel(const DenseTransArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / a.nsl, sl = blockIdx.x - b * a.nsl;
  const int npo = a.Ho * a.Wo;
  float* ss = reinterpret_cast<float*>(smem + a.xbytes);
  dense_stage_norm(ss, a.scale, a.shift, a.C, tid);
  __syncthreads();

  T* orow = static_cast<T*>(a.out) + (size_t)b * npo * a.ldo;
  DenseSrc src{static_cast<const T*>(a.x) + (size_t)b * a.H * a.W * a.C, a.C, npo, a.C, a.W, a.Wo};
  DenseGemm g{a.w, a.C, a.N, sl * 128 + wave * 32, a.kc, a.mf};
  dense_gemm128<T, true>(smem, ss, src, g, tid, [&](int m0, int j, float4v c0, float4v c1) {
    const int p = m0 + 16 * j + col;
    dense_store_pair<T>(orow + (size_t)p * a.ldo, g.nb, a.N, q, p < npo, c0, c1);
  });
}

template <typename T>
static void dense_transition_launch_as(const DenseTransArgs& a, int B, int lds, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&dense_transition_kernel<T>), dense::kSmallBudget);
  hipLaunchKernelGGL((dense_transition_kernel<T>), dim3((unsigned)(B * a.nsl)), dim3(256), lds, st, a);
}

bool dense_transition_ok(int H, int W, int C, int ldo) {
  return H >= 2 && W >= 2 && C > 0 && C % 32 == 0 && C <= dense::kMaxCin && ldo % 8 == 0 && C / 2 <= ldo;
}

bool dense_transition_launch(const void* x, const float* scale, const float* shift, const void* w, void* out, int B,
                             int H, int W, int C, int ldo, bool f32, hipStream_t st) {
  if (B <= 0 || !dense_transition_ok(H, W, C, ldo)) return false;
  const int sz = f32 ? 4 : 2;
  DenseTransArgs a{};
  a.x = x; a.scale = scale; a.shift = shift; a.w = w; a.out = out;
  a.H = H; a.W = W; a.C = C; a.N = C / 2; a.Ho = H / 2; a.Wo = W / 2; a.ldo = ldo;
  a.nsl = (a.N + 127) / 128;
  a.mf = a.Ho * a.Wo > 16 ? 2 : 1;                            // four loads a slot: half of phase 1's chunk
  const int kcb = C * sz < dense::kMaxChunkBytes ? C * sz : dense::kMaxChunkBytes;
  a.kc = kcb / sz;
  a.xbytes = 16 * a.mf * (kcb + 16);
  const int lds = a.xbytes + 2 * C * 4;
  if (lds > dense::kSmallBudget || (long)B * a.nsl >= (1L << 31)) return false;
  if (f32) dense_transition_launch_as<float>(a, B, lds, st);
  else dense_transition_launch_as<half_t>(a, B, lds, st);
  return true;
}

// ---- max pool into a wider buffer ------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) maxpool_into_kernel(const T* x, T* buf, long total, int H, int W, int C, int Ho,
                                                           int Wo, int ldo, int k, int s, int pad) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename DenseFrag<T>::type V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = C / E;
  const int c = (int)(i % cv);
  long p = i / cv;
  const int wo = (int)(p % Wo);
  p /= Wo;
  const int ho = (int)(p % Ho), b = (int)(p / Ho);
  const int y0 = max(ho * s - pad, 0), y1 = min(ho * s - pad + k, H);
  const int x0 = max(wo * s - pad, 0), x1 = min(wo * s - pad + k, W);
  float m[E];
#pragma unroll
  for (int e = 0; e < E; ++e) m[e] = -INFINITY;
  for (int y = y0; y < y1; ++y)
    for (int xx = x0; xx < x1; ++xx) {
      const V v = *reinterpret_cast<const V*>(x + (((size_t)b * H + y) * W + xx) * C + c * E);
#pragma unroll
      for (int e = 0; e < E; ++e) m[e] = fmaxf(m[e], (float)v[e]);
    }
  V o;
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = (T)m[e];                 // exact: each is one of the inputs
  *reinterpret_cast<V*>(buf + (((size_t)b * Ho + ho) * Wo + wo) * ldo + c * E) = o;
}

bool maxpool_into_launch(const void* x, void* buf, int B, int H, int W, int C, int Ho, int Wo, int ldo, int k, int s,
                         int pad, bool f32, hipStream_t st) {
  if (B <= 0 || C <= 0 || C % 8 || ldo % 8 || C > ldo || Ho <= 0 || Wo <= 0 || k < 1 || s < 1 || pad < 0 || 2 * pad > k)
    return false;
  // every window holds an input pixel: its first row / column ho s - pad <= H - 1
  if ((Ho - 1) * s - pad >= H || (Wo - 1) * s - pad >= W) return false;
  const long total = (long)B * Ho * Wo * (C / (f32 ? 4 : 8));
  const long blocks = (total + 255) / 256;
  if (blocks >= (1L << 31)) return false;
  if (f32)
    hipLaunchKernelGGL((maxpool_into_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, st,
                       static_cast<const float*>(x), static_cast<float*>(buf), total, H, W, C, Ho, Wo, ldo, k, s, pad);
  else
    hipLaunchKernelGGL((maxpool_into_kernel<half_t>), dim3((unsigned)blocks), dim3(256), 0, st,
                       static_cast<const half_t*>(x), static_cast<half_t*>(buf), total, H, W, C, Ho, Wo, ldo, k, s, pad);
  return true;
}

// ---- norm5 + ReLU + global average pool --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) bn_relu_avgpool_kernel(const T* x, const float* scale, const float* shift, T* out,
                                                              int total, int HW, int C) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename DenseFrag<T>::type V;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = C / E, b = i / cv, c = (i - b * cv) * E;
  float sc[E], sh[E], sum[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    sc[e] = scale[c + e];
    sh[e] = shift[c + e];
    sum[e] = 0.f;
  }
  const T* xp = x + (size_t)b * HW * C + c;
  for (int p = 0; p < HW; ++p) {                              // pixel order: the same sum every run
    const V v = *reinterpret_cast<const V*>(xp + (size_t)p * C);
#pragma unroll
    for (int e = 0; e < E; ++e) sum[e] += fmaxf((float)v[e] * sc[e] + sh[e], 0.f);
  }
  const float inv = 1.f / (float)HW;
  V o;
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = (T)(sum[e] * inv);
  *reinterpret_cast<V*>(out + (size_t)b * C + c) = o;
}

bool bn_relu_avgpool_launch(const void* x, const float* scale, const float* shift, void* out, int B, int HW, int C,
                            bool f32, hipStream_t st) {
  if (B <= 0 || HW <= 0 || C <= 0 || C % 8) return false;
  const long total = (long)B * (C / (f32 ? 4 : 8));
  if (total >= (1L << 31)) return false;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (f32)
    hipLaunchKernelGGL((bn_relu_avgpool_kernel<float>), dim3(blocks), dim3(256), 0, st, static_cast<const float*>(x),
                       scale, shift, static_cast<float*>(out), (int)total, HW, C);
  else
    hipLaunchKernelGGL((bn_relu_avgpool_kernel<half_t>), dim3(blocks), dim3(256), 0, st, static_cast<const half_t*>(x),
                       scale, shift, static_cast<half_t*>(out), (int)total, HW, C);
  return true;
}

}  // namespace idunno
