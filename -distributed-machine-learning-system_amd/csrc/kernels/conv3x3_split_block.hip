// One ResNet layer-1 basic block, out = relu(conv_b(relu(conv_a(x))) + x), both convs
// 3x3 / stride 1 / pad 1, 64 -> 64 channels on split fp16, in ONE row-streaming launch:
// the intermediate y never leaves the CU.  The one-conv kernel (conv3x3_split.hip)
// run twice moves x, y (written), y (read), x (the residual) and out through memory.
//
// Roles.  One 512-thread workgroup per CU, 8 waves, 2 per SIMD.  Waves 0-3 are the
// PRODUCER (conv a), waves 4-7 the CONSUMER (conv b); wave w of a role owns output
// channels 16 (w % 4) .. + 15 of its conv and holds their A fragments (144 VGPRs) for
// the whole launch.  A SIMD hosts one producer and one consumer wave, which share its
// MFMA pipe.
//
// Rings.  Two 5-row LDS rings in the layout of the one-conv kernel (256-byte pixels,
// slot = chunk ^ ((2 col) & 15), RC columns): the x ring is filled by the row DMA
// (split over all 8 waves), the y ring by the producer's epilogue (scale, bias, ReLU,
// split_f16x4, range guard, then a 16-byte LDS store at the swizzled slot).  y-ring
// columns 0 and W+1 .. RC-1 are cleared once per launch and never stored to; a y row
// outside the image is written as zeros instead of being computed.
//
// Steps.  A band of output rows [y0, y1) of one image runs steps s = y0-1 .. y1+1, one
// workgroup barrier each.  At step s
//   * the producer makes y row s from x rows s-1 .. s+1.  Its tail fragment pairs rows
//     (s, s+1) when s - y0 is even, so it also reads x row s+2 and y row s is complete
//     when step s ends (pairing (s-1, s) as the one-conv kernel does would finish row
//     s-1's columns 48.. one step late, and the consumer would need a sixth y row);
//   * x row s+3 is landing by DMA (rows s-1 .. s+2 in use: 5 ring rows);
//   * the consumer makes out row r = s-2 from y rows r-1 .. r+1, its tail pairing rows
//     (r-1, r) when r - y0 is odd.  Producer 4-fragment steps fall on consumer
//     3-fragment steps: every step issues 7 fragments' MFMAs on each SIMD.
//   y rows live in a step: s-3 .. s+1 (even) or s-4 .. s (odd): 5 ring rows.
// The residual x row s-2 has left the x ring by then (its slot takes row s+3), so the
// consumer loads it from global memory when the row starts, as the one-conv kernel
// does: the same CU DMA'd that row five steps earlier, an L2 hit.
//
// Each accumulator receives the MFMAs of the one-conv kernel in the same order (tap,
// channel block, hi*hi, hi*lo, lo*hi) and y is rounded by the same split_f16x4, so the
// result is bit-identical to the two launches whatever the band split.
#include "conv3x3_split_c64.h"

namespace idunno {

namespace c64b {
constexpr int RING = 5;
constexpr int YR = RING * c64s::RB;         // the y ring follows the x ring
constexpr int BIAS = 2 * RING * c64s::RB;   // conv a's 64 biases, then conv b's
constexpr int LDS = BIAS + 512;             // 154,112 B: one workgroup per CU
}  // namespace c64b

struct C64bArgs {
  const half_t* x;      // split [B][H][W][128]; also the residual
  const half_t* wa;     // split weights [64][9 * 128] of conv a
  const half_t* wb;     // ... and conv b
  const float* ba;      // [64]
  const float* bb;      // [64]
  half_t* out;          // split [B][H][W][128]
  int B, H, W, nrows;
  float scale_a, scale_b;
  int* ovf;             // split range guard flag or nullptr
};

__device__ __forceinline__ void lds_write_b128(uint32_t addr, u32x4_sw v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}

template <int D>
__global__ void __launch_bounds__(512, 1) conv3x3_split_c64_block_kernel(const C64bArgs a) {
  using namespace c64s;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2, cw = wave & 3;         // 0 producer (conv a), 1 consumer (conv b)
  const int frow = lane & 15, q = lane >> 4;
  const int r_begin = (int)((long long)blockIdx.x * a.nrows / gridDim.x);
  const int r_end = (int)((long long)(blockIdx.x + 1) * a.nrows / gridDim.x);
  if (r_begin >= r_end) return;              // uniform

  // ---- A fragments of this wave's 16 couts of its conv: [tap][block][hi|lo] ----
  half8v fa[9][2][2];
  {
    const half_t* wr = (role ? a.wb : a.wa) + (size_t)(cw * 16 + frow) * (9 * PIX) + q * 8;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int p = 0; p < 2; ++p) fa[t][cb][p] = *reinterpret_cast<const half8v*>(wr + t * PIX + cb * 64 + p * 32);
  }
  const int n0 = cw * 16 + 4 * q;              // this lane's 4 output channels (C/D layout)
  if (tid < 32)
    *reinterpret_cast<float4v*>(smem + c64b::BIAS + 16 * tid) =
        *reinterpret_cast<const float4v*>((tid < 16 ? a.ba : a.bb) + 4 * (tid & 15));
  const float* bias_lds = reinterpret_cast<const float*>(smem + c64b::BIAS) + role * 64 + n0;
  const uint32_t ring = lds_addr(smem) + (uint32_t)(role * c64b::YR);   // the ring this role READS
  const uint32_t yring = lds_addr(smem) + (uint32_t)c64b::YR;
  // y ring: zeros in every column once; only columns 1 .. W are ever stored to
  for (int i = tid; i < c64b::RING * RC * 16; i += 512) lds_write_b128(yring + 16 * i, u32x4_sw{0u, 0u, 0u, 0u});
  const auto x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, 0x7fffffff, 0x00020000);
  uint32_t voff[2];
  c64s_row_offsets<512>(a.W, tid, voff);
  // per-lane LDS byte offset of column col0 + kw, chunk 4c + q (conv3x3_split.hip)
  auto col_off = [&](int col) {
    const int x = (2 * col) & 15;
    return (uint32_t)(col * 256 + (((x >> 2) & 3) << 6) + (((q ^ x) & 3) << 4));
  };
  uint32_t loff[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) loff[kw] = col_off(frow + kw);
  const uint32_t tshift = frow < 8 ? 48u * 256u : 40u * 256u;
  const int tcol = 48 + (frow & 7);            // the tail fragment's output column
  const int tailn = a.W - 48;                  // valid tail columns per row (1..8)
  // the producer's store: its lane's 16 bytes are global chunk sc of the pixel
  // (split_off_q in 16-byte units), at y-ring column (image column + 1)
  const int sc = split_off_q(cw * 16, q) >> 3;
  auto ystore_off = [&](int col) { return (uint32_t)(col * 256 + (c64s_slot(sc, col) << 4)); };

  // One row of one role.  c = the row (producer: y row s; consumer: out row s-2); the
  // role's input ring holds rows c-2 .. c+2 at ((row + 2 RING) % RING).  `pair`: the
  // tail fragment covers two rows, lanes 0-7 the earlier one: (c, c+1) for the
  // producer, (c-1, c) for the consumer.
  auto row = [&](auto rolet, auto nft, int b, int c, bool pair) {
    constexpr int ROLE = decltype(rolet)::value;
    constexpr int NF = decltype(nft)::value;       // 3: fragments 0-2; 4: + the tail
    constexpr int NG = 18 * NF;
    const bool tother = pair && (ROLE ? frow < 8 : frow >= 8);   // lanes of the pair's other row
    const int trow = tother ? (ROLE ? c - 1 : c + 1) : c;
    const bool tok = (frow & 7) < tailn && (pair || frow < 8);
    const uint32_t rowpix = (uint32_t)((b * a.H + c) * a.W);
    const uint32_t tpix = (uint32_t)((b * a.H + trow) * a.W + min(tcol, a.W - 1));
    uint32_t rb5[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) rb5[i] = ring + (uint32_t)(((c - 2 + i + 2 * c64b::RING) % c64b::RING) * RB);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) asm volatile("" : "+v"(loff[kw]));
    float4v rw[ROLE ? NF : 1];
    if constexpr (ROLE == 1) {
      // residual (x) of the row's fragments -> registers when the row starts
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const uint32_t off = (f < 3 ? rowpix + 16 * f + frow : tpix) * PIX + split_off_q(n0 - 4 * q, q);
        rw[f] = gload_f4_untracked(a.x + off);
      }
    }
    float4v acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = float4v{0.f, 0.f, 0.f, 0.f};
    half8v bf[D][2];
    auto issue = [&](int g, int buf) {
      const int t = g / (2 * NF), cb = (g / NF) & 1, F = g % NF;
      const int kh = t / 3, kw = t - 3 * kh;
      uint32_t base;
      if (F < 3) {
        base = rb5[kh + 1] + loff[kw];
      } else {
        uint32_t ts = tshift;
        asm volatile("" : "+v"(ts));
        base = (tother ? rb5[ROLE ? kh : kh + 2] : rb5[kh + 1]) + ts + loff[kw];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) bf[buf][p] = lds_read_frag(base ^ (uint32_t)((2 * cb + p) << 6), F);
    };
#pragma unroll
    for (int p = 0; p < D - 1; ++p) issue(p, p);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int buf = g % D;
      if (g + D - 1 < NG) {
        issue(g + D - 1, (g + D - 1) % D);
        c64s_wait_groups<D - 1>();
      } else {
        c64s_wait_groups<0>();
      }
      lds_tie(bf[buf][0]);
      lds_tie(bf[buf][1]);
      const int t = g / (2 * NF), cb = (g / NF) & 1, F = g % NF;
      float4v& cc = acc[F];
      cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[t][cb][0], bf[buf][0], cc, 0, 0, 0);
      cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[t][cb][0], bf[buf][1], cc, 0, 0, 0);
      cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[t][cb][1], bf[buf][0], cc, 0, 0, 0);
    }
    // ---- epilogue: scale, bias (+ residual), ReLU, split; to the y ring or to out ----
    if constexpr (ROLE == 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int f = 0; f < NF; ++f) reg_tie(rw[f]);
    }
    const float scale = ROLE ? a.scale_b : a.scale_a;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      float4v v = acc[f] * scale + *reinterpret_cast<const float4v*>(bias_lds);
      if constexpr (ROLE == 1) {
        half4v h, l;
        split_swap_in(rw[f], h, l);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)h[e] + (float)l[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      half4v h, l;
      split_f16x4(v, h, l);
      const u32x4_sw o = split_swap_out(h, l);     // the lane swap runs on every lane
      if (f == 3 && !tok) continue;                // a tail lane with column >= W never stores
      split_guard(a.ovf, v);
      if constexpr (ROLE == 1) {
        const uint32_t off = (f < 3 ? rowpix + 16 * f + frow : tpix) * PIX + split_off_q(n0 - 4 * q, q);
        *reinterpret_cast<u32x4_sw*>(a.out + off) = o;
      } else {
        const int yr = f < 3 ? c : trow;
        const int col = (f < 3 ? 16 * f + frow : tcol) + 1;
        lds_write_b128(yring + (uint32_t)(((yr + 2 * c64b::RING) % c64b::RING) * RB) + ystore_off(col), o);
      }
    }
  };

  for (int r = r_begin; r < r_end;) {           // one band per image the range touches
    const int b = r / a.H;
    const int y0 = r - b * a.H;
    const int y1 = min(a.H, y0 + (r_end - r));
    r += y1 - y0;
    const int ylast = min(a.H - 1, y1);         // the last y row that is computed
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // previous band's ring reads are done; first: the y ring is clear
#pragma unroll
    // x rows y0-2 .. y0+1: the first step, s = y0-1, makes y row y0-1 from x rows s-1 .. s+1 =
    // y0-2 .. y0 (rb5[1..3]), and row s+2 = y0+1 must have landed when the step starts
    for (int i = -2; i <= 1; ++i)
      c64s_load_row<512>(smem, x_rsrc, voff, a.H, a.W, b, y0 + i, (y0 + i + 2 * c64b::RING) % c64b::RING, tid);
    bool stored = false;                        // this wave's previous step ended with >= NST global stores
    for (int s = y0 - 1; s <= y1 + 1; ++s) {
      // Counted waits, per role.  x row s+2 (DMA issued in step s-1, or by the band's
      // prologue) must have landed.  Producer waves issue nothing but the DMAs
      // (their epilogue stores go to LDS): vmcnt(0) waits for exactly those.  A
      // consumer wave's step is DMA, residual loads, [vmcnt(0) before the epilogue],
      // >= NST stores: after such a step its DMAs are already retired and vmcnt(NST)
      // leaves the stores in flight; after a step without an epilogue (the band's
      // first three steps) it waits vmcnt(0) like the producer.  lgkmcnt(0): the
      // producer's y-ring stores are done before the barrier publishes them.  The
      // barrier also ends every wave's reads of x row s-2 and of the y rows of step
      // s-1, whose slots this step's DMA and y stores take.
      if (stored) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NST) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stored = false;
      if (s + 3 <= ylast + 1) c64s_load_row<512>(smem, x_rsrc, voff, a.H, a.W, b, s + 3, (s + 3 + 2 * c64b::RING) % c64b::RING, tid);
      if (role == 0) {
        if (s > y1) continue;                   // the consumer's last row: nothing to produce
        if ((unsigned)s >= (unsigned)a.H) {     // y row -1 or H: zeros in columns 1 .. W
          const uint32_t zr = yring + (uint32_t)(((s + 2 * c64b::RING) % c64b::RING) * RB);
          for (int i = (tid & 255) + 16; i < (a.W + 1) * 16; i += 256) lds_write_b128(zr + 16 * i, u32x4_sw{0u, 0u, 0u, 0u});
          continue;
        }
        const bool first = s >= y0 && ((s - y0) & 1) == 0;   // tail step: rows (s, s+1), or s alone
        if (first || s < y0) row(c64s_nf<0>{}, c64s_nf<4>{}, b, s, first && s + 1 <= ylast);
        else row(c64s_nf<0>{}, c64s_nf<3>{}, b, s, false);
      } else {
        const int c = s - 2;
        if (c < y0) continue;
        const bool pair = ((c - y0) & 1) != 0;               // tail of rows (c-1, c)
        if (pair || c == y1 - 1) row(c64s_nf<1>{}, c64s_nf<4>{}, b, c, pair);
        else row(c64s_nf<1>{}, c64s_nf<3>{}, b, c, false);
        stored = true;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

bool conv3x3_split_c64_block_supported(int B, int H, int W, int C, int Cout) {
  return conv3x3_split_c64_supported(H, W, C, Cout) && B >= 1 && (long)B * H * W * c64s::PIX * 2 < (1L << 31);
}

// the batches the fused kernel takes by default: where the one-conv launcher runs two
// workgroups per CU (below that it picks one per CU, and the unfused path stays)
bool conv3x3_split_c64_block_default(int B, int H) { return B * H >= 16 * device_cu_count(); }

bool conv3x3_split_c64_block_launch(const half_t* x, const half_t* wa, const float* ba, float scale_a, const half_t* wb,
                                    const float* bb, float scale_b, half_t* out, int B, int H, int W, int* ovf,
                                    hipStream_t st, int max_grid) {
  if (!conv3x3_split_c64_block_supported(B, H, W, 64, 64)) return false;
  C64bArgs a;
  a.x = x;
  a.wa = wa;
  a.wb = wb;
  a.ba = ba;
  a.bb = bb;
  a.out = out;
  a.B = B;
  a.H = H;
  a.W = W;
  a.nrows = B * H;
  a.scale_a = scale_a;
  a.scale_b = scale_b;
  a.ovf = ovf;
  // one workgroup per CU, equal row shares; max_grid > 0 caps the grid (tests: bands
  // that span several images on small tensors)
  int grid = device_cu_count();
  if (max_grid > 0 && grid > max_grid) grid = max_grid;
  if (grid > a.nrows) grid = a.nrows;
  ensure_lds_attr(reinterpret_cast<const void*>(conv3x3_split_c64_block_kernel<3>), c64b::LDS);
  hipLaunchKernelGGL((conv3x3_split_c64_block_kernel<3>), dim3(grid), dim3(512), c64b::LDS, st, a);
  return true;
}

}  // namespace idunno
