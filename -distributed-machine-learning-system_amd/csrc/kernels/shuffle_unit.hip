// ShuffleNetV2 for gfx950: a whole unit -- channel split, 1x1, depthwise 3x3, 1x1, concat and channel shuffle -- in
// one launch, both strides, NHWC fp16 or true fp32 by template.  Activations are [B, H, W, Cp] in logical channel
// order with Cp = roundup(c, 8) (only width 116 pads); shuffle_math.h has the widths, the band planner and the LDS
// layout.
//
//   stride 1:  out[2i] = x[i]                      out[2i + 1] = relu(W2 dw(relu(W1 x[h:c] + b1)) + b2)[i]
//   stride 2:  out[2i] = relu(Wp dw1_s2(x) + bp)[i]  out[2i + 1] = relu(W2 dw_s2(relu(W1 x + b1)) + b2)[i]
//
// shuffle_unit_kernel<T, STRIDE>: a workgroup (4 waves) owns a band of R output rows of one image -- at 7x7 of
// several images, so that a GEMM's M reaches four fragments.
//
//   1. Stage.  The band's input rows (R + 2 or 2 R + 1, clipped to the image) go to LDS with 16-byte loads, pixel
//      pitch Kx sz + 16.  Stride 1 stages channels [k0, Cp) only, k0 = floor8(h): what pw1 walks.  The rows of W1
//      for channels outside [h, c) are zero, so h = 58 needs no unaligned access and an input pad channel (any
//      finite value) reaches nothing.  Slots past Cp and past the pixel list are stored as zero.
//   2. pw1 on the MFMA, weights as the A operand so that a lane of the accumulator holds 4 channels of one pixel.
//      relu(acc + b1) goes to the LDS map, rows x (W + 2) pixels of hp channels.  The map is cleared first and
//      only in-image pixels are written: its border and the rows above and below the image are true zeros, the
//      depthwise conv's padding, not relu(b1).
//   3. Depthwise 3x3 from the map, f32 accumulate, bias, no activation, one rounding, into pw2's operand in LDS.  A
//      thread owns a pixel and a 16-byte channel chunk.  Stride 2 runs a second pass straight off the staged input
//      for branch 1 (the image border is tested, not padded).
//   4. pw2 (and branch 1's 1x1) on the MFMA.  Stride 2 runs branch 1 first and parks relu(acc + bp), rounded, in
//      LDS.  pw2's operand and that parked output lie over the staged input, which is dead by then.
//   5. Epilogue of pw2.  A lane holds y[i .. i + 3] of one pixel; it fetches the four even-channel values -- x1
//      straight from global memory at stride 1 (a copy, hence bit-exact), branch 1 from LDS at stride 2 --
//      interleaves them in registers and stores output channels [2 i, 2 i + 8): one 16-byte store in fp16, two
//      in fp32.  i >= h is forced to zero on both sides, so the pad channels [c, Cp) are written as zero.
//
// GEMM shape: a wave owns 16-channel fragments wave, wave + 4, ... of N; for each it walks the pixel list in
// groups of 8 fragments, K innermost, the next K step's weights loaded under this step's MFMAs.  Weights come
// from global memory (L2): row-major [hp, K], zero-padded, 16 bytes a lane.
#include "../common.h"
#include "../kernels.h"
#include "../launch_util.h"
#include "../shuffle_math.h"

namespace idunno {

template <typename T>
struct ShufFrag;
template <>
struct ShufFrag<half_t> {
  typedef half8v type;
  typedef half4v out4;
  static __device__ __forceinline__ float4v mma(half8v a, half8v b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct ShufFrag<float> {
  typedef float4v type;
  typedef float4v out4;
  static __device__ __forceinline__ float4v mma(float4v a, float4v b, float4v c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], c, 0, 0, 0);
    return c;
  }
};

template <typename V, typename T>
__device__ __forceinline__ V shuf_zero() {
  V z;
#pragma unroll
  for (int e = 0; e < 16 / (int)sizeof(T); ++e) z[e] = (T)0.f;
  return z;
}

struct ShuffleArgs {
  const void* x;
  void* out;
  ShuffleUnitWeights w;
  int B, H, W, h;
  shuffle::Plan p;
};

constexpr int kShufMP = 8;      // pixel fragments a weight fragment meets before it is loaded again

// acc(nf, m) = sum_k w[16 nf + n][k] bs[m][k]: N = 16 nfn channels, K = Kp, M = npix pixels of `pitch` bytes in LDS
// (rows up to the next multiple of 16 exist).  epi(nf, m, acc): lane (col, q) holds channels 16 nf + 4 q .. + 3 of
// pixel m = 16 fragment + col; called for m < npix only.
template <typename T, typename Epi>
__device__ __forceinline__ void shuf_gemm(const void* w, int Kp, int nfn, const char* bs, int pitch, int npix, int wave,
                                          int col, int q, Epi epi) {
  constexpr int E = 16 / (int)sizeof(T), KS = 4 * E;
  typedef typename ShufFrag<T>::type V;
  const int nks = Kp / KS, npf = (npix + 15) / 16;
  const float4v zf = {0.f, 0.f, 0.f, 0.f};
  const char* brow = bs + col * pitch + q * 16;
  for (int nf = wave; nf < nfn; nf += 4) {                          // wave-uniform
    const T* wrow = static_cast<const T*>(w) + (size_t)(nf * 16 + col) * Kp + q * E;
    for (int pf0 = 0; pf0 < npf; pf0 += kShufMP) {
      float4v acc[kShufMP];
#pragma unroll
      for (int j = 0; j < kShufMP; ++j) acc[j] = zf;
      V a = *reinterpret_cast<const V*>(wrow);
      for (int ks = 0; ks < nks; ++ks) {
        V an = a;
        if (ks + 1 < nks) an = *reinterpret_cast<const V*>(wrow + (ks + 1) * KS);
#pragma unroll
        for (int j = 0; j < kShufMP; ++j) {
          if (pf0 + j >= npf) continue;                             // wave-uniform
          const V b = *reinterpret_cast<const V*>(brow + (pf0 + j) * 16 * pitch + ks * 64);
          acc[j] = ShufFrag<T>::mma(a, b, acc[j]);
        }
        a = an;
      }
#pragma unroll
      for (int j = 0; j < kShufMP; ++j) {
        const int m = (pf0 + j) * 16 + col;
        if (pf0 + j < npf && m < npix) epi(nf, m, acc[j]);
      }
    }
  }
}

// depthwise 3x3 over `npo` output pixels x `kch` 16-byte channel chunks; tap(p, t, v) fetches pixel p's tap t chunk
// (false: the tap is padding); f32 accumulate from the bias, one rounding, dst pixel pitch `pitch`
template <typename T, typename Tap>
__device__ __forceinline__ void shuf_dw(const void* wd, const float* bd, int ld, int kch, int npo, char* dst, int pitch,
                                        int tid, Tap tap) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename ShufFrag<T>::type V;
  for (int i = tid; i < npo * kch; i += 256) {
    const int p = i / kch, ch = i - p * kch;
    float s[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = bd[ch * E + e];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      V v;
      if (!tap(p, t, ch, v)) continue;
      const V wv = *reinterpret_cast<const V*>(static_cast<const T*>(wd) + t * ld + ch * E);
#pragma unroll
      for (int e = 0; e < E; ++e) s[e] += (float)v[e] * (float)wv[e];
    }
    V o;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = (T)s[e];
    *reinterpret_cast<V*>(dst + p * pitch + ch * 16) = o;
  }
}

template <typename T, int STRIDE>
__global__ void __launch_bounds__(256) shuffle_unit_kernel(const ShuffleArgs a) {
  constexpr int SZ = (int)sizeof(T), E = 16 / SZ;
  typedef typename ShufFrag<T>::type V;
  typedef typename ShufFrag<T>::out4 O4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const shuffle::Plan& P = a.p;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int grp = blockIdx.x / P.nbands, band = blockIdx.x - grp * P.nbands;
  const int b0 = grp * P.imgs, nimg = min(P.imgs, a.B - b0);        // images of this workgroup
  const int r0 = band * P.R, rows = min(P.R, P.Ho - r0);            // output rows
  const int W2 = a.W + 2;
  // input rows [ilo, ihi); map row 0 is input row mtop (stride 1: r0 - 1, stride 2: 2 r0 - 1)
  const int mtop = STRIDE * r0 - 1;
  const int ilo = max(mtop, 0), ihi = min(STRIDE * (r0 + rows - 1) + 2, a.H), rin = ihi - ilo;
  const int mrows = shuffle::in_rows(P.R, STRIDE);
  const int npin = nimg * rin * a.W, npo = nimg * rows * P.Wo;
  char* xs = smem;
  char* map = smem + P.map_off;
  char* a2 = smem;                                                  // over the staged input, once it is dead
  char* o1 = smem + P.o1_off;
  const V zero = shuf_zero<V, T>();
  const T* xg = static_cast<const T*>(a.x);
  const int nfn = P.hp / 16;

  // ---- 1. stage the input rows, clear the map ----------------------------------------------------------------------
  {
    const int kch = P.Kx / E, total = shuffle::rup(npin, 16) * kch;
    for (int i = tid; i < total; i += 256) {
      const int m = i / kch, ch = i - m * kch, k = P.k0 + ch * E;
      V v = zero;
      if (m < npin && k < P.cpin) {
        const shuffle::Pix px = shuffle::pix_of(m, rin, a.W);
        v = *reinterpret_cast<const V*>(xg + (((size_t)(b0 + px.img) * a.H + ilo + px.r) * a.W + px.c) * P.cpin + k);
      }
      *reinterpret_cast<V*>(xs + m * P.px + ch * 16) = v;
    }
    for (int i = tid * 16; i < P.imgs * mrows * W2 * P.pm; i += 256 * 16) *reinterpret_cast<V*>(map + i) = zero;
  }
  __syncthreads();

  // ---- 2. pw1: staged pixels -> map ---------------------------------------------------------------------------------
  shuf_gemm<T>(a.w.w1, P.Kx, nfn, xs, P.px, npin, wave, col, q, [&](int nf, int m, float4v acc) {
    const shuffle::Pix px = shuffle::pix_of(m, rin, a.W);
    const int n = nf * 16 + 4 * q;
    const float4v bq = *reinterpret_cast<const float4v*>(a.w.b1 + n);
    O4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (T)fmaxf(acc[e] + bq[e], 0.f);
    *reinterpret_cast<O4*>(map + ((px.img * mrows + ilo + px.r - mtop) * W2 + px.c + 1) * P.pm + n * SZ) = o;
  });
  if constexpr (STRIDE == 2) {
    // branch 1's depthwise conv, straight off the staged input
    shuf_dw<T>(a.w.wd1, a.w.bd1, P.Kx, P.Kx / E, npo, smem + P.a1_off, P.px, tid, [&](int p, int t, int ch, V& v) {
      const shuffle::Pix px = shuffle::pix_of(p, rows, P.Wo);
      const int dy = t / 3, dx = t - 3 * dy, iy = 2 * (r0 + px.r) - 1 + dy, ix = 2 * px.c - 1 + dx;
      if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) return false;
      v = *reinterpret_cast<const V*>(xs + ((px.img * rin + iy - ilo) * a.W + ix) * P.px + ch * 16);
      return true;
    });
  }
  __syncthreads();

  // ---- 3. the depthwise 3x3 over the map -> pw2's operand, over the dead staged input -------------------------------
  shuf_dw<T>(a.w.wd, a.w.bd, P.hp, P.hp / E, npo, a2, P.pm, tid, [&](int p, int t, int ch, V& v) {
    const shuffle::Pix px = shuffle::pix_of(p, rows, P.Wo);
    const int dy = t / 3, dx = t - 3 * dy;
    v = *reinterpret_cast<const V*>(map + ((px.img * mrows + STRIDE * px.r + dy) * W2 + STRIDE * px.c + dx) * P.pm +
                                    ch * 16);
    return true;
  });
  __syncthreads();

  // ---- 4. stride 2: branch 1's 1x1 -> LDS, behind pw2's operand ------------------------------------------------------
  if constexpr (STRIDE == 2) {
    shuf_gemm<T>(a.w.wp1, P.Kx, nfn, smem + P.a1_off, P.px, npo, wave, col, q, [&](int nf, int m, float4v acc) {
      const int n = nf * 16 + 4 * q;
      const float4v bq = *reinterpret_cast<const float4v*>(a.w.bp1 + n);
      O4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)fmaxf(acc[e] + bq[e], 0.f);
      *reinterpret_cast<O4*>(o1 + m * P.pm + n * SZ) = o;
    });
    __syncthreads();
  }

  // ---- 5. pw2 and the shuffled store ---------------------------------------------------------------------------------
  T* og = static_cast<T*>(a.out);
  shuf_gemm<T>(a.w.w2, P.hp, nfn, a2, P.pm, npo, wave, col, q, [&](int nf, int m, float4v acc) {
    const int n = nf * 16 + 4 * q;
    if (2 * n >= P.cp) return;
    const shuffle::Pix px = shuffle::pix_of(m, rows, P.Wo);
    const size_t pix = ((size_t)(b0 + px.img) * P.Ho + r0 + px.r) * P.Wo + px.c;
    O4 ev;
    if constexpr (STRIDE == 1) ev = *reinterpret_cast<const O4*>(xg + pix * P.cpin + n);   // n + 3 < cp / 2 + 3 <= cpin
    else ev = *reinterpret_cast<const O4*>(o1 + m * P.pm + n * SZ);
    const float4v bq = *reinterpret_cast<const float4v*>(a.w.b2 + n);
    T o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = n + e < a.h;
      o[2 * e] = ok ? ev[e] : (T)0.f;
      o[2 * e + 1] = ok ? (T)fmaxf(acc[e] + bq[e], 0.f) : (T)0.f;
    }
    T* dst = og + pix * P.cp + 2 * n;
#pragma unroll
    for (int v = 0; v < 8 / E; ++v) {
      V ov;
#pragma unroll
      for (int e = 0; e < E; ++e) ov[e] = o[v * E + e];
      *reinterpret_cast<V*>(dst + v * E) = ov;
    }
  });
}

bool shuffle_plan(int H, int W, int cin, int c, int stride, bool f32, int out[9]) {
  shuffle::Plan p;
  if (!shuffle::plan(H, W, cin, c, stride, f32, p)) return false;
  out[0] = p.R; out[1] = p.nbands; out[2] = p.imgs; out[3] = p.lds;
  out[4] = p.hp; out[5] = p.Kx; out[6] = p.cp; out[7] = p.cpin;
  shuffle::Plan whole = p;
  out[8] = shuffle::layout(H, W, stride, p.Ho, 1, whole);        // what one band an image would take
  return true;
}

template <typename T, int STRIDE>
static void shuffle_unit_launch_as(const ShuffleArgs& a, unsigned blocks, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&shuffle_unit_kernel<T, STRIDE>), shuffle::kBudget);
  hipLaunchKernelGGL((shuffle_unit_kernel<T, STRIDE>), dim3(blocks), dim3(256), a.p.lds, st, a);
}

bool shuffle_unit_launch(const void* x, void* out, const ShuffleUnitWeights& w, int B, int H, int W, int cin, int c,
                         int stride, bool f32, hipStream_t st) {
  ShuffleArgs a{};
  if (B <= 0 || !shuffle::plan(H, W, cin, c, stride, f32, a.p)) return false;
  if (!w.w1 || !w.b1 || !w.wd || !w.bd || !w.w2 || !w.b2) return false;
  if (stride == 2 && (!w.wd1 || !w.bd1 || !w.wp1 || !w.bp1)) return false;
  const long blocks = (long)((B + a.p.imgs - 1) / a.p.imgs) * a.p.nbands;
  if (blocks >= (1L << 31)) return false;
  a.x = x; a.out = out; a.w = w;
  a.B = B; a.H = H; a.W = W; a.h = c / 2;
  if (f32) {
    if (stride == 1) shuffle_unit_launch_as<float, 1>(a, (unsigned)blocks, st);
    else shuffle_unit_launch_as<float, 2>(a, (unsigned)blocks, st);
  } else {
    if (stride == 1) shuffle_unit_launch_as<half_t, 1>(a, (unsigned)blocks, st);
    else shuffle_unit_launch_as<half_t, 2>(a, (unsigned)blocks, st);
  }
  return true;
}

}  // namespace idunno
