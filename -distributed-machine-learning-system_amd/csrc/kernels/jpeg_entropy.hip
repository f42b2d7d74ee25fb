// Device entropy stage of the JPEG source: Huffman streams -> quantised DCT
// coefficients, the opt-in counterpart of runtime/jpeg_entropy.cpp.
//
// Huffman decoding is serial per stream, so the parallelism is over images: one
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
// The host (bindings.cpp jpeg_entropy_gpu) has checked every descriptor against
// the three buffers with jpeg_huff_check before the launch; inside a span the
// core checks every access itself.
#include <hip/hip_runtime.h>

#include "../jpeg_huff_core.h"
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

}  // namespace

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
