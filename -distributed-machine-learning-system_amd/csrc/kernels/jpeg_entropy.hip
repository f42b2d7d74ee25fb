// Device entropy stage of the JPEG source: Huffman streams -> quantised DCT
// coefficients, the opt-in counterpart of runtime/jpeg_entropy.cpp.
//
// Two kernels.  jpeg_entropy_kernel (entropy_on="gpu"): Huffman decoding is serial
// per stream, so the parallelism is over images: one
// lane decodes one whole scan with the host/device core of jpeg_huff_core.h.
// Workgroups are a single wave, so that a batch of B images spreads over
// ceil(B / 64) CUs instead of filling a few.  The lanes of a wave walk different
// streams: loads are per-lane word reads of each image's own byte span (sequential
// per lane, so each 128-byte line is fetched once and then hit in L1/L2) and
// table lookups in the shared table buffer in global memory (datasets use a
// handful of table sets, ~12 KB each, which stay cache-resident; 64 distinct sets
// would not fit the LDS of one wave's workgroup).  Coefficient stores are scattered
// int16 writes into a buffer the launcher zeroed.
//
// jpeg_entropy_par_kernel (entropy_on="gpu_parallel", further down) decodes one
// image on a whole workgroup instead.  jpeg_entropy_prog_kernel
// (progressive="native") decodes the progressive files of a batch, one lane
// per image like the first, in either device form.  jpeg_entropy_rst_kernel
// (restart="intervals", last) decodes the baseline files with a restart interval,
// one lane per interval, in either device form as well.
//
// Four-component files (CMYK / YCCK, colorspace="auto") are decoded by the first and the
// third kernel only: the packer never marks one for the sub-stream or the interval kernel,
// whose state and item layouts stay those of one and three components.
//
// The host (bind_jpeg.cpp jpeg_entropy_gpu / jpeg_entropy_gpu_parallel) has checked every descriptor against
// the three buffers with jpeg_huff_check before the launch (the progressive entries'
// scan ranges and table indices with jpeg_huff_prog_check, the restart-interval
// entries' work items with jpeg_huff_rst_check); inside a span the core checks
// every access itself.
#include <hip/hip_runtime.h>

#include "../jpeg_huff_core.h"
#include "../jpeg_huff_par.h"
#include "../jpeg_huff_prog.h"
#include "../jpeg_huff_rst.h"
#include "../kernels.h"

namespace idunno {

namespace {

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes,
                                                          const JpegHuffSet* __restrict__ sets,
                                                          const JpegHuffDesc* __restrict__ desc,
                                                          int16_t* __restrict__ coef, int* __restrict__ status, int n) {
  const int i = (int)(blockIdx.x * 64u + threadIdx.x);
  if (i >= n) return;
  const JpegHuffDesc& d = desc[i];
  if (d.gpu != 1) return;
  status[i] = jpeg_huff_decode_scan(d, reinterpret_cast<const uint32_t*>(bytes + d.byte_off), sets[d.set_idx],
                                    coef + d.coef_base);
}

// One image on the lanes of a whole workgroup (entropy_on="gpu_parallel"): the
// self-synchronising sub-streams of jpeg_huff_par.h.  Workgroup i takes entry i of
// the batch (gpu == 2; any other entry ends it at once); thread t takes the
// sub-streams t, t + T, ... of kJpegParSubBits bits, so any stream length runs on
// the fixed T = kJpegParThreads.  Everything the threads of an image exchange goes
// through a barrier of their own workgroup: no workgroup waits for another one.
//   * The image's table set (11.6 KB) is copied to LDS once: a lane step is a chain
//     of dependent table lookups, and unlike the one-lane kernel all lanes of the
//     workgroup share one set.
//   * The state (6 words per sub-stream: two entry buffers, so that a round reads
//     only what the previous round wrote, blocks completed, three DC sums) lives in
//     LDS up to kParLdsSubs sub-streams (128 KiB of scan data), else in the image's
//     span of the global scratch buffer.
//   * Rounds: at most min(sub-streams, kJpegParMaxRounds); __syncthreads_or carries
//     "some entry changed".  A lane step is divergent by nature (each lane walks its
//     own bits); a lane whose entry did not change skips its step, so from the
//     second round on most lanes of a wave are idle and the few that run finish
//     sooner than a full pass.  Not converged: kJpegHuffUnsynced, nothing written.
//   * Prefix of blocks and DC sums: each thread sums a contiguous share, reads the
//     shares before its own from LDS, and rewrites its share as exclusive prefixes.
//   * Write pass: strict decode with every store checked; any refusal, or a stream
//     that ends before the scan's last block, is JPEG_CORRUPT.
constexpr uint32_t kParLdsSubs = 1024;

__global__ __launch_bounds__(kJpegParThreads) void jpeg_entropy_par_kernel(
    const uint8_t* __restrict__ bytes, const JpegHuffSet* __restrict__ sets, const JpegHuffDesc* __restrict__ desc,
    const JpegParDesc* __restrict__ par, int16_t* __restrict__ coef, int* __restrict__ status,
    uint32_t* __restrict__ scratch, int n) {
  __shared__ JpegHuffSet set_lds;
  __shared__ uint32_t st_lds[kJpegParStateWords * kParLdsSubs];
  __shared__ uint32_t part[kJpegParThreads][4];
  const int i = (int)blockIdx.x;
  if (i >= n) return;
  const JpegHuffDesc& d = desc[i];
  if (d.gpu != 2) return;                        // uniform: the whole workgroup leaves
  const JpegParDesc& p = par[i];
  const uint32_t t = threadIdx.x, T = kJpegParThreads;
  {
    static_assert(sizeof(JpegHuffSet) % 4 == 0, "copied by words");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&sets[d.set_idx]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&set_lds);
    for (uint32_t q = t; q < sizeof(JpegHuffSet) / 4; q += T) dst[q] = src[q];
  }
  JpegParCtx x;
  x.d = &d;
  x.p = &p;
  x.words = reinterpret_cast<const uint32_t*>(bytes + d.byte_off);
  x.set = &set_lds;
  x.sub_bits = kJpegParSubBits;
  x.nsub = jpeg_par_nsub(p.bit_len, kJpegParSubBits);
  x.st = x.nsub <= kParLdsSubs ? st_lds : scratch + p.scratch_off;
  x.coef = coef + d.coef_base;
  jpeg_par_init(x, t, T);
  __syncthreads();
  const uint32_t R = x.nsub < kJpegParMaxRounds ? x.nsub : kJpegParMaxRounds;
  int cur = 0;
  bool converged = false;
  for (uint32_t r = 0; r < R; ++r) {
    const bool any = jpeg_par_round(x, cur, t, T);
    if (!__syncthreads_or(any ? 1 : 0)) {        // also the barrier between this round's writes and the next one's reads
      converged = true;
      break;
    }
    cur ^= 1;
  }
  if (!converged) {
    if (t == 0) status[i] = kJpegHuffUnsynced;
    return;
  }
  jpeg_par_partial(x, t, T, part[t]);
  __syncthreads();
  uint32_t base[4] = {0u, 0u, 0u, 0u};
  for (uint32_t u = 0; u < t; ++u)
    for (int q = 0; q < 4; ++q) base[q] += part[u][q];
  jpeg_par_scan(x, t, T, base);
  // the last thread's base + its own share: the blocks the whole stream holds
  int bad = (t == T - 1 && base[0] + part[t][0] < p.total_blocks) ? 1 : 0;
  __syncthreads();
  if (jpeg_par_write(x, cur, t, T) != kJpegHuffOk) bad = 1;
  bad = __syncthreads_or(bad);
  if (t == 0) status[i] = bad ? kJpegHuffCorrupt : kJpegHuffOk;
}

// Progressive files (progressive="native", gpu == 3): one lane decodes every scan of
// one image with the core of jpeg_huff_prog.h, in workgroups of one wave like
// jpeg_entropy_kernel.  The grid runs over `list`, the compact indices of the
// batch's progressive entries, so a batch with a few progressive files among many
// baseline ones does not launch waves of idle lanes.  A refinement scan reads back
// the coefficients the same lane stored in an earlier scan of the same launch:
// plain loads and stores of one thread to its own span, in program order.  Tables
// are single JpegHuffTabs (1.5 KB) in global memory, shared by the images that
// carry identical ones.
__global__ __launch_bounds__(64) void jpeg_entropy_prog_kernel(const uint8_t* __restrict__ bytes,
                                                               const JpegHuffTab* __restrict__ tabs, int ntabs,
                                                               const JpegProgScan* __restrict__ scans, long long nscans,
                                                               const JpegHuffDesc* __restrict__ desc, int n,
                                                               const int* __restrict__ list, int nlist,
                                                               int16_t* coef, int* __restrict__ status) {
  const int j = (int)(blockIdx.x * 64u + threadIdx.x);
  if (j >= nlist) return;
  const int i = list[j];
  if (i < 0 || i >= n) return;
  const JpegHuffDesc& d = desc[i];
  if (d.gpu != 3) return;
  status[i] = jpeg_prog_decode_image(d, scans, nscans, reinterpret_cast<const uint32_t*>(bytes + d.byte_off), tabs,
                                     ntabs, coef + d.coef_base);
}

// Restart-interval files (restart="intervals", gpu == 4): one lane decodes one restart
// interval with the core of jpeg_huff_rst.h, over the flattened item list of the whole
// batch, in workgroups of one wave like jpeg_entropy_kernel so that a small batch spreads
// over the CUs.  The items of one image sit on consecutive lanes, and the core's flat
// one-symbol-per-trip loop keeps a wave on the same instructions across block and MCU
// boundaries.  A wave may hold items of several images with different table sets, so the
// tables stay in global memory as in the one-lane kernel.  Intervals write disjoint
// blocks of the image's span.  A lane whose interval is refused raises the image's status
// with an atomic max; a lane that accepts writes nothing, so status is zero on entry (the
// caller's torch.zeros).  No barrier, no LDS, no lane or workgroup waits for another.
__global__ __launch_bounds__(64) void jpeg_entropy_rst_kernel(const uint8_t* __restrict__ bytes,
                                                              const JpegHuffSet* __restrict__ sets,
                                                              const JpegHuffDesc* __restrict__ desc,
                                                              const JpegRstItem* __restrict__ items, int nitems,
                                                              int16_t* __restrict__ coef, int* status, int n) {
  const long long j = (long long)blockIdx.x * 64 + threadIdx.x;
  if (j >= nitems) return;
  const JpegRstItem it = items[j];
  if (it.entry < 0 || it.entry >= n) return;
  const JpegHuffDesc& d = desc[it.entry];
  if (d.gpu != 4) return;
  const int st = jpeg_huff_decode_interval(d, reinterpret_cast<const uint32_t*>(bytes + d.byte_off), sets[d.set_idx],
                                           coef + d.coef_base, it.byte_begin, it.mcu_first, it.index);
  if (st != kJpegHuffOk) atomicMax(&status[it.entry], kJpegHuffCorrupt);
}

}  // namespace

void jpeg_entropy_rst_launch(const uint8_t* bytes, const JpegHuffSet* sets, const JpegHuffDesc* desc,
                             const JpegRstItem* items, int nitems, int16_t* coef, int* status, int n,
                             hipStream_t st) {
  if (nitems <= 0 || n <= 0) return;
  hipLaunchKernelGGL(jpeg_entropy_rst_kernel, dim3((unsigned)(((long long)nitems + 63) / 64)), dim3(64), 0, st, bytes,
                     sets, desc, items, nitems, coef, status, n);
}

void jpeg_entropy_prog_launch(const uint8_t* bytes, const JpegHuffTab* tabs, int ntabs, const JpegProgScan* scans,
                              long long nscans, const JpegHuffDesc* desc, int n, const int* list, int nlist,
                              int16_t* coef, int* status, hipStream_t st) {
  if (nlist <= 0) return;
  hipLaunchKernelGGL(jpeg_entropy_prog_kernel, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, st, bytes, tabs, ntabs,
                     scans, nscans, desc, n, list, nlist, coef, status);
}

void jpeg_entropy_par_launch(const uint8_t* bytes, const JpegHuffSet* sets, const JpegHuffDesc* desc,
                             const JpegParDesc* par, int16_t* coef, int* status, uint32_t* scratch, int n,
                             hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(jpeg_entropy_par_kernel, dim3((unsigned)n), dim3(kJpegParThreads), 0, st, bytes, sets, desc, par,
                     coef, status, scratch, n);
}

void jpeg_entropy_zero_launch(int16_t* coef, long long coef_elems, hipStream_t st) {
  if (coef_elems <= 0) return;
  (void)hipMemsetAsync(coef, 0, (size_t)coef_elems * sizeof(int16_t), st);
}

void jpeg_entropy_launch(const uint8_t* bytes, const JpegHuffSet* sets, const JpegHuffDesc* desc, int16_t* coef,
                         int* status, int n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, bytes, sets, desc, coef,
                     status, n);
}

}  // namespace idunno
