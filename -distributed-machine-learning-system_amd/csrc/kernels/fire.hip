// SqueezeNet for gfx950: the Fire module in one launch, and the classifier head (1x1 conv + ReLU +
// global average pool) without its [B, H, W, N] tensor.  NHWC fp16 or true fp32 by template.
//
//   s = relu(Ws x + bs)                                   x [B, H, W, Cin],  s [B, H, W, S]
//   y = concat(relu(W1 s + b1), relu(W3 (*)3x3,pad1 s + b3))   y [B, H, W, E1 + E3]
//
// fire_kernel<T, S>: a workgroup (4 waves) owns one image and a band of R output rows.
//
//   * Squeeze.  The band's input rows plus one halo row each side, clipped to the image, are one
//     contiguous pixel range of x (rows are full width).  It is walked in chunks of 16 MF pixels,
//     staged as conv1x1_narrow.hip stages its tile (16-byte loads and stores, zeros from Cin to Kp
//     and past the range), and multiplied on the MFMA with Ws as the A operand (streamed from L2,
//     next step prefetched), so a lane ends with four consecutive squeeze channels of one pixel.
//     relu(. + bs), rounded to T, goes to the s region of LDS: (rows + 2) x (W + 2) pixels of
//     PS = S sizeof(T) + 16 bytes.  The region is cleared first and only in-image pixels are
//     written: column -1, column W and the rows outside the image stay zero.  The 3x3's zero
//     padding therefore applies to s (a halo squeezed from zero-padded x would be relu(bs)), and
//     s never reaches HBM.  The recomputed halo rows (2 / R of the squeeze, itself 15 - 20 % of the
//     module's MACs) are the only redundant work.
//   * Expand.  One implicit GEMM over K = 9 S, tap-major (k = tap S + c), with We as the A operand
//     and the band's output pixels as the B operand, read from the s region only: lane (col, q) of
//     K step ks reads the 16-byte chunk g = 4 ks + q, i.e. tap g / CPT (CPT = chunks a tap) at
//     ((dy (W + 2) + dx) PS + 16 (g % CPT)) past its pixel's window origin.  The 1x1 expand's rows
//     of We hold W1 in the centre tap's K slice and the loop walks only the K steps that cover
//     [4 S, 5 S): no staging pass of its own.  9 S is ragged against fp16's 32-wide step at S = 16
//     and 48 (144 -> 160, 432 -> 448): the pad exists in the packed weights (zeros) and as one
//     64-byte zero slot in LDS that the pad chunks read, so no stale LDS meets a zero weight.
//     fp32's step is 16 and 9 S is always whole.
//     Waves are WN x WM like the narrow kernel: WN = 1, 2 or 4 over pairs of 16-channel fragments
//     (3x3 pairs first, they are 9 x the 1x1's work), WM = 4 / WN over pixel fragments.  A wave
//     keeps a pair's two weight fragments of a K step in registers (the next step prefetched under
//     this step's MFMAs) and uses them for up to MP = 8 pixel fragments; a band of more fragments
//     takes several passes.  Weights read by a module: (E1 + 9 E3) S elements, <= 328 KB in fp16.
//   * Epilogue: bias and ReLU on the transposed accumulator; fp32 stores float4s, fp16 trades
//     halves within the pair (split_swap_out) for one 16-byte store a lane, the 1x1 expand at
//     channels [0, E1), the 3x3 at [E1, E1 + E3) of the one output tensor.  E1 and E3 are multiples
//     of 16: a half pair at the end of either expand is predicated off, never padded in HBM.
//   * LDS pitches.  x chunk rows: Kp sizeof(T) + 16, an odd number of 16-byte slots as in
//     conv1x1_narrow.hip.  s pixels: PS = 48 / 80 / 112 / 144 bytes (fp16, S = 16 .. 64) and
//     80 / 144 / 208 / 272 (fp32): 3, 5, 7, 9 and 5, 9, 13, 17 slots, all odd, so the 16 lanes of a
//     ds_read_b128 lane group (16 consecutive pixels of a row, one chunk) fall on 16 different
//     slots of the 64 banks.  A fragment that wraps to the next row skips two pixels and can meet
//     one two-way conflict (lanes 14 pixels apart); staging stores write consecutive chunks.
//   * Band height and occupancy (fire_plan).  fp16: 80 KiB a workgroup, two a CU.  The x chunk
//     takes at most 34 KiB (MF 4, 2 or 1), the rest holds R + 2 rows of s, R <= 16, balanced over
//     the image: 55 x 55 x (S 16, Cin 96) is four bands of 14 rows (halo 2 / 14) in 55.8 KiB,
//     13 x 13 x (S 64, Cin 512) one band in 64.2 KiB.  fp32 takes the same 80 KiB plan where it
//     gives >= 8 rows a band and an image of <= 16 rows one band: two workgroups a CU for the
//     S = 16 modules, S = 32 at 27 x 27 and S = 48 at 13 x 13.  Else it plans for 160 KiB (x chunk
//     <= 68 KiB), one workgroup a CU: S = 32 at 55 x 55, S >= 48 at 27 x 27, S = 64 at 13 x 13
//     (124.3 KiB at fire9).  docs/KERNELS.md lists every module.  W <= 96 always plans (one row a
//     band at the widest); W <= 64 leaves at least three.
//
// conv1x1_pool_kernel<T>: out[b, n] = mean_p relu(x[b, p, :] w[n, :] + bias[n]), fp32 out.  A
// workgroup owns an image and 128 output channels (a pair a wave); the image's pixels are staged
// in chunks of 16 MF, each lane adds relu(acc + bias) of its pixels -- only rows below H W, a
// padding row would add relu(bias) -- into two float4s in fragment order, then the 16 pixel lanes
// are summed by a fixed xor butterfly: the same order every run, no atomics.
#include "../common.h"
#include "../kernels.h"
#include "../launch_util.h"

namespace idunno {

template <typename T>
struct FireFrag;
template <>
struct FireFrag<half_t> {
  typedef half8v type;
  typedef half4v out4;
  static __device__ __forceinline__ float4v mma(half8v a, half8v b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct FireFrag<float> {
  typedef float4v type;
  typedef float4v out4;
  static __device__ __forceinline__ float4v mma(float4v a, float4v b, float4v c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], c, 0, 0, 0);
    return c;
  }
};

template <typename V, typename T>
__device__ __forceinline__ V fire_zero() {
  V z;
#pragma unroll
  for (int e = 0; e < 16 / (int)sizeof(T); ++e) z[e] = (T)0.f;
  return z;
}

// rows [m0, m0 + nrows) of x[mend, ldx] -> LDS rows of `pitch` bytes: K channels, zeros up to Kp and past mend
template <typename T>
__device__ __forceinline__ void fire_stage_rows(char* smem, const T* xb, int ldx, int m0, int mend, int nrows, int K,
                                                int Kp, int pitch, int tid) {
  constexpr int E = 16 / (int)sizeof(T);
  typedef typename FireFrag<T>::type V;
  const int cpr = Kp / E, kvc = K / E, total = nrows * cpr;
  constexpr int BATCH = 4;
  for (int i0 = tid; i0 < total; i0 += 256 * BATCH) {
    V v[BATCH];
    int off[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + 256 * j;
      v[j] = fire_zero<V, T>();
      off[j] = -1;
      if (i < total) {
        const int m = i / cpr, c = i - m * cpr;
        off[j] = m * pitch + c * 16;
        if (m0 + m < mend && c < kvc) v[j] = *reinterpret_cast<const V*>(xb + (size_t)(m0 + m) * ldx + c * E);
      }
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
      if (off[j] >= 0) *reinterpret_cast<V*>(smem + off[j]) = v[j];
  }
}

struct FireArgs {
  const void* x;       // [B, H, W, Cin]
  const void* ws;      // [S, Kp] squeeze weights, zero from Cin to Kp
  const float* bs;     // [S]
  const void* we;      // [E1 + E3, KpE]: rows < E1 hold W1 at k in [4 S, 5 S), the rest W3 tap-major; zero from 9 S
  const float* be;     // [E1 + E3]
  void* y;             // [B, H, W, E1 + E3]
  int B, H, W, Cin, Kp, E1, E3, KpE;
  int R, nbands;       // band height, bands an image
  int mf;              // squeeze chunk: 16 mf pixels
  int xbytes;          // bytes of the x chunk region (the zero slot and the s region follow)
};

constexpr int kFireMP = 8;          // pixel fragments a pass of the expand
constexpr int kFireMaxW = 96;

template <typename T, int S>
__global__ void __launch_bounds__(256) fire_kernel(const FireArgs a) {
  constexpr int SZ = (int)sizeof(T), E = 16 / SZ, KS = 4 * E, CPT = S / E;
  constexpr int PS = S * SZ + 16;
  constexpr bool F16 = SZ == 2;
  typedef typename FireFrag<T>::type V;
  typedef typename FireFrag<T>::out4 O4;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / a.nbands, band = blockIdx.x - b * a.nbands;
  const int r0 = band * a.R, rows = min(a.R, a.H - r0);
  const int W2 = a.W + 2;
  char* zs = smem + a.xbytes;       // 64 zero bytes
  char* ss = zs + 64;               // s: [rows + 2][W + 2][PS]
  const V zero = fire_zero<V, T>();

  for (int i = tid * 16; i < 64 + (rows + 2) * W2 * PS; i += 256 * 16) *reinterpret_cast<V*>(zs + i) = zero;

  // ---- squeeze: image rows [rlo, rhi) -> s rows rlo - (r0 - 1) ... --------------------------------------------
  {
    constexpr int NFR = S / 16, WN = NFR >= 3 ? 4 : NFR, WM = 4 / WN;
    const int wn = wave / WM, wm = wave % WM;
    const int rlo = max(r0 - 1, 0), rhi = min(r0 + rows + 1, a.H);
    const int npix = (rhi - rlo) * a.W;
    const T* xb = static_cast<const T*>(a.x) + ((size_t)b * a.H + rlo) * a.W * a.Cin;
    const int pitch = a.Kp * SZ + 16, nks = a.Kp / KS;
    const char* brow = smem + col * pitch + q * 16;
    const T* w0 = static_cast<const T*>(a.ws) + (size_t)((wn % NFR) * 16 + col) * a.Kp + q * E;
    const float4v bq = *reinterpret_cast<const float4v*>(a.bs + (wn % NFR) * 16 + 4 * q);
    for (int m0 = 0; m0 < npix; m0 += 16 * a.mf) {
      fire_stage_rows<T>(smem, xb, a.Cin, m0, npix, 16 * a.mf, a.Cin, a.Kp, pitch, tid);
      __syncthreads();
      if (wn < NFR) {                                         // wave-uniform (S = 48: the fourth wave rests)
        float4v acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = float4v{0.f, 0.f, 0.f, 0.f};
        V an = *reinterpret_cast<const V*>(w0);
        for (int ks = 0; ks < nks; ++ks) {
          const V av = an;
          if (ks + 1 < nks) an = *reinterpret_cast<const V*>(w0 + (ks + 1) * KS);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j >= a.mf || j % WM != wm) continue;         // wave-uniform
            const V bx = *reinterpret_cast<const V*>(brow + 16 * j * pitch + ks * (KS * SZ));
            acc[j] = FireFrag<T>::mma(av, bx, acc[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= a.mf || j % WM != wm) continue;
          const int m = m0 + 16 * j + col;
          if (m >= npix) continue;
          const int pr = m / a.W, pc = m - pr * a.W;
          O4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (T)fmaxf(acc[j][e] + bq[e], 0.f);
          *reinterpret_cast<O4*>(ss + ((rlo + pr - (r0 - 1)) * W2 + pc + 1) * PS + (wn * 16 + 4 * q) * SZ) = o;
        }
      }
      __syncthreads();
    }
  }

  // ---- expand: both convs read s from LDS --------------------------------------------------------------------
  const int npo = rows * a.W, nfrag = (npo + 15) / 16;
  const int np3 = (a.E3 + 31) / 32, np1 = (a.E1 + 31) / 32;
  const int WN = np3 >= 3 ? 4 : np3, WM = 4 / WN, wmask = WM - 1;
  const int wm = wave & wmask, wn = wave / WM;
  const int ctot = a.E1 + a.E3;
  const size_t ybase = ((size_t)b * a.H + r0) * a.W;          // first output pixel of the band

  for (int pi = wn; pi < np3 + np1; pi += WN) {               // wave-uniform
    const bool is3 = pi < np3;
    const int nb = is3 ? a.E1 + pi * 32 : (pi - np3) * 32;
    const int lim = is3 ? ctot : a.E1;
    const int ks0 = is3 ? 0 : (4 * S) / KS, ks1 = is3 ? a.KpE / KS : (5 * S + KS - 1) / KS;
    const bool ok0 = nb + col < lim, ok1 = nb + 16 + col < lim;
    const T* w0 = static_cast<const T*>(a.we) + (size_t)(nb + col) * a.KpE + q * E;
    const T* w1 = w0 + (size_t)16 * a.KpE;
    const int n0 = nb + 4 * q, n1 = n0 + 16;
    const float4v zf = {0.f, 0.f, 0.f, 0.f};
    const float4v b0 = n0 < lim ? *reinterpret_cast<const float4v*>(a.be + n0) : zf;
    const float4v b1 = n1 < lim ? *reinterpret_cast<const float4v*>(a.be + n1) : zf;

    for (int f0 = 0; f0 < nfrag; f0 += kFireMP) {
      int base[kFireMP];                                      // window origin of this lane's pixel of fragment f0 + j
      float4v acc[kFireMP][2];
#pragma unroll
      for (int j = 0; j < kFireMP; ++j) {
        const int p = (f0 + j) * 16 + col, pp = p < npo ? p : 0;
        const int r = pp / a.W, c = pp - r * a.W;
        base[j] = (r * W2 + c) * PS;
        acc[j][0] = acc[j][1] = zf;
      }
      V a0n = ok0 ? *reinterpret_cast<const V*>(w0 + ks0 * KS) : zero;
      V a1n = ok1 ? *reinterpret_cast<const V*>(w1 + ks0 * KS) : zero;
      for (int ks = ks0; ks < ks1; ++ks) {
        const V a0 = a0n, a1 = a1n;
        if (ks + 1 < ks1) {
          a0n = ok0 ? *reinterpret_cast<const V*>(w0 + (ks + 1) * KS) : zero;
          a1n = ok1 ? *reinterpret_cast<const V*>(w1 + (ks + 1) * KS) : zero;
        }
        const int g = ks * 4 + q, tap = g / CPT, cc = g - tap * CPT;
        const int dy = tap / 3, dx = tap - 3 * dy;
        const int off = (dy * W2 + dx) * PS + cc * 16;
        const bool kpad = tap >= 9;                           // fp16, S = 16 | 48: the last step's tail
#pragma unroll
        for (int j = 0; j < kFireMP; ++j) {
          if (f0 + j >= nfrag || (j & wmask) != wm) continue; // wave-uniform
          const V bx = *reinterpret_cast<const V*>(kpad ? zs : ss + base[j] + off);
          acc[j][0] = FireFrag<T>::mma(a0, bx, acc[j][0]);
          acc[j][1] = FireFrag<T>::mma(a1, bx, acc[j][1]);
        }
      }

      // lane (col, q) holds channels nb + 16 f + 4 q .. + 3 of output pixel 16 (f0 + j) + col of the band
#pragma unroll
      for (int j = 0; j < kFireMP; ++j) {
        if (f0 + j >= nfrag || (j & wmask) != wm) continue;   // wave-uniform
        reg_tie(acc[j][0]);
        reg_tie(acc[j][1]);
        const int p = (f0 + j) * 16 + col;
        const bool mok = p < npo;
        const size_t rowoff = (ybase + p) * ctot;
        float4v v0 = acc[j][0] + b0, v1 = acc[j][1] + b1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v0[e] = fmaxf(v0[e], 0.f);
          v1[e] = fmaxf(v1[e], 0.f);
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
          if (mok && off < lim) *reinterpret_cast<u32x4_sw*>(static_cast<half_t*>(a.y) + rowoff + off) = sw;
        } else {
          float* yp = static_cast<float*>(a.y) + rowoff;
          if (mok && n0 < lim) *reinterpret_cast<float4v*>(yp + n0) = v0;
          if (mok && n1 < lim) *reinterpret_cast<float4v*>(yp + n1) = v1;
        }
      }
    }
  }
}

// ---- band height, chunk size and LDS bytes of a Fire launch ------------------------------------------------------
struct FirePlan {
  int R, mf, xbytes, lds;
};

static bool fire_plan_in(int H, int W, int Kp, int S, int sz, int budget, int xcap, FirePlan& p) {
  const int pitch = Kp * sz + 16, rowb = (W + 2) * (S * sz + 16);
  int mf = 4;
  while (mf > 1 && 16 * mf * pitch > xcap) mf /= 2;
  const int xbytes = 16 * mf * pitch;
  int rmax = (budget - xbytes - 64) / rowb - 2;
  if (rmax < 1) return false;
  rmax = rmax < 16 ? rmax : 16;
  rmax = rmax < H ? rmax : H;
  const int nb = (H + rmax - 1) / rmax;
  p.R = (H + nb - 1) / nb;
  p.mf = mf;
  p.xbytes = xbytes;
  p.lds = xbytes + 64 + (p.R + 2) * rowb;
  return true;
}

static bool fire_plan(int H, int W, int Cin, int S, bool f32, FirePlan& p) {
  const int Kp = conv1x1_narrow_kpad(Cin, f32), sz = f32 ? 4 : 2;
  if (fire_plan_in(H, W, Kp, S, sz, 80 * 1024, 34 * 1024, p) && (!f32 || p.R >= (H <= 16 ? H : 8))) return true;
  return f32 && fire_plan_in(H, W, Kp, S, sz, 160 * 1024, 68 * 1024, p);
}

int fire_kpad(int S, bool f32) { return conv1x1_narrow_kpad(9 * S, f32); }

bool fire_ok(int H, int W, int Cin, int S, int E1, int E3, bool f32) {
  if (H <= 0 || W <= 0 || W > kFireMaxW || Cin <= 0 || Cin % 16 || Cin > 512) return false;
  if (S != 16 && S != 32 && S != 48 && S != 64) return false;
  if (E1 <= 0 || E3 <= 0 || E1 % 16 || E3 % 16 || E1 > 256 || E3 > 256) return false;
  FirePlan p;
  return fire_plan(H, W, Cin, S, f32, p);
}

int fire_max_w() { return kFireMaxW; }

template <typename T, int S>
static void fire_launch_as(const FireArgs& a, int lds, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&fire_kernel<T, S>), 160 * 1024);
  hipLaunchKernelGGL((fire_kernel<T, S>), dim3((unsigned)(a.B * a.nbands)), dim3(256), lds, st, a);
}

template <typename T>
static void fire_launch_s(const FireArgs& a, int S, int lds, hipStream_t st) {
  if (S == 16) fire_launch_as<T, 16>(a, lds, st);
  else if (S == 32) fire_launch_as<T, 32>(a, lds, st);
  else if (S == 48) fire_launch_as<T, 48>(a, lds, st);
  else fire_launch_as<T, 64>(a, lds, st);
}

bool fire_launch(const void* x, const void* ws, const float* bs, const void* we, const float* be, void* y, int B, int H,
                 int W, int Cin, int S, int E1, int E3, bool f32, hipStream_t st) {
  FirePlan p;
  if (B <= 0 || !fire_ok(H, W, Cin, S, E1, E3, f32) || !fire_plan(H, W, Cin, S, f32, p)) return false;
  FireArgs a{};
  a.x = x; a.ws = ws; a.bs = bs; a.we = we; a.be = be; a.y = y;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.E1 = E1; a.E3 = E3;
  a.Kp = conv1x1_narrow_kpad(Cin, f32);
  a.KpE = fire_kpad(S, f32);
  a.R = p.R;
  a.nbands = (H + p.R - 1) / p.R;
  a.mf = p.mf;
  a.xbytes = p.xbytes;
  if ((long)B * a.nbands >= (1L << 31)) return false;
  if (f32) fire_launch_s<float>(a, S, p.lds, st);
  else fire_launch_s<half_t>(a, S, p.lds, st);
  return true;
}

// ---- classifier head: 1x1 conv + ReLU + global average pool ----------------------------------------------------
struct PoolHeadArgs {
  const void* x;       // [B, HW, K]
  const void* w;       // [N, Kp], zero from K
  const float* bias;   // [N]
  float* out;          // [B, N]
  int HW, K, Kp, N, mf;
  int nsl;             // 128-channel slices of N
};

constexpr int kPoolHeadLds = 16 * (1280 * 4 + 16);

template <typename T>
__global__ void __launch_bounds__(256) conv1x1_pool_kernel(const PoolHeadArgs a) {
  constexpr int SZ = (int)sizeof(T), E = 16 / SZ, KS = 4 * E;
  typedef typename FireFrag<T>::type V;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / a.nsl, nb = ((blockIdx.x - b * a.nsl) * 4 + wave) * 32;
  const bool active = nb < a.N;                               // wave-uniform
  const int pitch = a.Kp * SZ + 16, nks = a.Kp / KS;
  const T* xb = static_cast<const T*>(a.x) + (size_t)b * a.HW * a.K;
  const char* brow = smem + col * pitch + q * 16;
  const bool ok0 = nb + col < a.N, ok1 = nb + 16 + col < a.N;
  const T* w0 = static_cast<const T*>(a.w) + (size_t)(nb + col) * a.Kp + q * E;
  const T* w1 = w0 + (size_t)16 * a.Kp;
  const int n0 = nb + 4 * q, n1 = n0 + 16;
  const float4v zf = {0.f, 0.f, 0.f, 0.f};
  const float4v b0 = n0 < a.N ? *reinterpret_cast<const float4v*>(a.bias + n0) : zf;
  const float4v b1 = n1 < a.N ? *reinterpret_cast<const float4v*>(a.bias + n1) : zf;
  const V zero = fire_zero<V, T>();
  float4v s0 = zf, s1 = zf;

  for (int m0 = 0; m0 < a.HW; m0 += 16 * a.mf) {
    fire_stage_rows<T>(smem, xb, a.K, m0, a.HW, 16 * a.mf, a.K, a.Kp, pitch, tid);
    __syncthreads();
    if (active) {
      float4v acc[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = zf;
      V a0n = ok0 ? *reinterpret_cast<const V*>(w0) : zero;
      V a1n = ok1 ? *reinterpret_cast<const V*>(w1) : zero;
      for (int ks = 0; ks < nks; ++ks) {
        const V a0 = a0n, a1 = a1n;
        if (ks + 1 < nks) {
          a0n = ok0 ? *reinterpret_cast<const V*>(w0 + (ks + 1) * KS) : zero;
          a1n = ok1 ? *reinterpret_cast<const V*>(w1 + (ks + 1) * KS) : zero;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= a.mf) continue;                            // wave-uniform
          const V bx = *reinterpret_cast<const V*>(brow + 16 * j * pitch + ks * (KS * SZ));
          acc[j][0] = FireFrag<T>::mma(a0, bx, acc[j][0]);
          acc[j][1] = FireFrag<T>::mma(a1, bx, acc[j][1]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= a.mf || m0 + 16 * j + col >= a.HW) continue; // rows past H W add nothing, not relu(bias)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0[e] += fmaxf(acc[j][0][e] + b0[e], 0.f);
          s1[e] += fmaxf(acc[j][1][e] + b1[e], 0.f);
        }
      }
    }
    __syncthreads();
  }
  // the 16 pixel lanes of a lane group: a fixed butterfly
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0[e] += __shfl_xor(s0[e], o, kWave);
      s1[e] += __shfl_xor(s1[e], o, kWave);
    }
  }
  if (active && col == 0) {
    const float inv = 1.f / (float)a.HW;
    float* op = a.out + (size_t)b * a.N;
    if (n0 < a.N) *reinterpret_cast<float4v*>(op + n0) = s0 * inv;
    if (n1 < a.N) *reinterpret_cast<float4v*>(op + n1) = s1 * inv;
  }
}

template <typename T>
static void pool_head_launch_as(const PoolHeadArgs& a, int B, int lds, hipStream_t st) {
  ensure_lds_attr(reinterpret_cast<const void*>(&conv1x1_pool_kernel<T>), kPoolHeadLds);
  hipLaunchKernelGGL((conv1x1_pool_kernel<T>), dim3((unsigned)(B * a.nsl)), dim3(256), lds, st, a);
}

bool conv1x1_pool_launch(const void* x, const void* w, const float* bias, float* out, int B, int HW, int K, int N,
                         bool f32, hipStream_t st) {
  if (B <= 0 || B >= (1 << 24) || HW <= 0 || K <= 0 || N <= 0 || K % 8 || N % 8 || K > 1280 || N > 1280) return false;
  PoolHeadArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.out = out;
  a.HW = HW; a.K = K; a.N = N;
  a.Kp = conv1x1_narrow_kpad(K, f32);
  const int pitch = a.Kp * (f32 ? 4 : 2) + 16;
  int mf = 4;
  while (mf > 1 && (16 * mf * pitch > kPoolHeadLds || 16 * (mf / 2) >= HW)) mf /= 2;
  a.mf = mf;
  a.nsl = (N + 127) / 128;
  const int lds = 16 * mf * pitch;
  if (lds > kPoolHeadLds) return false;
  if (f32) pool_head_launch_as<float>(a, B, lds, st);
  else pool_head_launch_as<half_t>(a, B, lds, st);
  return true;
}

}  // namespace idunno
