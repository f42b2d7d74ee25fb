// Shared by the bind_*.cpp families: stream / launch checks, the per-device zero
// buffers, the split range guard, and the operand checks every entry point runs
// before it launches anything (a malformed launch on a shared MI355X box can
// fault the whole node).
//
// Everything declared here without a body is DEFINED ONCE in binding_util.cpp and
// must stay that way -- never `static` or `inline` in this header: zero_buffer and
// zero_f32 own function-local static state (the never-freed per-device buffers),
// and the split guard is thread_local.  A per-translation-unit copy of the guard
// would be set from one file and read as null in another, which silently disables
// the fp16-range guard of every split kernel.
#pragma once
#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "kernels.h"
#include "launch_util.h"

namespace idunno {

hipStream_t cur_stream();                 // PyTorch's *current* HIP stream (graph capture, side streams)
void check_launch(const char* what);      // every launch is checked
torch::Tensor zero_buffer(const torch::Device& dev);            // 256 zero bytes per device, never freed
torch::Tensor zero_f32(const torch::Device& dev, int64_t n);    // >= n fp32 zeros per device, never freed

// Split range guard (common.h split_guard): the int32 flag this thread's split
// launches write to when a value leaves fp16's range; null when unset.
void set_split_guard(c10::optional<torch::Tensor> flag);
int* split_guard_for(const torch::Device& dev);

// Kernel choice is a pure function of each call's arguments (no process-global
// switches): `tile` forces a kernel, `ksplit` forces split-K slices, `form` a stem
// kernel form, `route` (a per-runner policy, bits below) opts a call out of the
// specialised kernels for whole-graph A/Bs.
extern const int kRouteNoBand;         // no band-staged 3x3 kernel (tile 70)
extern const int kRouteNoC64;          // no row-streaming 3x3 64->64 kernels (tile 50)
extern const int kRouteNoStream1x1;    // no streaming 1x1 kernels (tile 80)
extern const int kRouteLegacySmallM;   // split convs: the round-5 small-M rules -- A/B arm of the round-6 rules
extern const int kRouteC64TwoPerCU;    // row-streaming 64->64 kernel: always two workgroups per CU (A/B arm)
extern const int kRouteBandW7;         // the band-staged 3x3 at W 7 too (the round-5 rule, A/B arm)
extern const int kRouteNoBandW28;      // no band-staged 3x3 at W 28 (ResNet layer2, A/B arm)

// One call per operand: a GPU tensor on `dev` (the first operand passes its own
// device) of dtype `dt` and rank `rank` (-1: the caller bounds numel instead),
// contiguous unless `contig` is false (views go through nhwc_pixel_stride).
void check_operand(const torch::Tensor& t, const char* name, at::ScalarType dt, int rank, const torch::Device& dev,
                   bool contig = true);
// Pixel stride (elements) of an NHWC view whose channels are contiguous and whose
// pixels are equally spaced: a channel slice of a wider tensor is read in place.
int64_t nhwc_pixel_stride(const torch::Tensor& t, const char* what);
// The validated caller-owned `out` (e.g. a batch slice of a bigger tensor), or a fresh tensor.
torch::Tensor optional_out(const c10::optional<torch::Tensor>& out, const torch::Device& dev, at::ScalarType dt,
                           at::IntArrayRef shape);
// Data pointer of the optional residual (null when absent) after its checks; with
// `pixel_stride` the binding reads NHWC views in place and gets the stride back.
const void* optional_res(const c10::optional<torch::Tensor>& res, const torch::Device& dev, at::ScalarType dt,
                         at::IntArrayRef shape, int64_t* pixel_stride = nullptr);
// x2 [B, H, W, .] must be the block input at `stride` of x1's [B, Ho, Wo, .] resolution (dual 1x1 convs)
void check_strided_input(const torch::Tensor& x2, int B, int Ho, int Wo, int64_t stride);
// Packed-row geometry of an RGB stem (preprocess_pack3* and conv2d_pack3*): row copies, elements per
// copy row, 16-byte chunks per kernel row
void pack3_geometry(int W, int KW, int stride, int pad, int elem_bytes, int& nc, int& wp, int& cpk);
// Device-side window of a resident image shard (bind_stem.cpp has the contract):
// returns the start pointer or null, B = images this launch, max_start the clamp.
const long long* window_args(const torch::Tensor& img, const c10::optional<torch::Tensor>& start, int64_t batch,
                             int64_t window, int64_t sub, int& B, long long& max_start);

// ConvArgs / ConvF32Args fields every conv binding fills the same way
template <class Args>
void fill_conv_geometry(Args& a, int B, int H, int W, int C, int Ho, int Wo, int Cout, int ldy, int KH, int KW,
                        int stride, int pad, long M, int Kpad, bool relu) {
  a.B = B; a.H = H; a.W = W; a.C = C;
  a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.ldy = ldy;
  a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
  a.M = (int)M;
  a.Kpad = Kpad;
  a.relu = relu ? 1 : 0;
}

// An FC layer as a 1x1 conv on K slices of each row (ldx = K), all `splits` slices
// in one launch into fp32 partials [splits, M, N] with a zero bias
template <class Args>
void fill_linear_splitk(Args& a, int64_t M, int64_t K, int64_t N, int64_t splits, const torch::Tensor& zero_bias,
                        torch::Tensor& part) {
  a.bias = zero_bias.data_ptr<float>();
  a.res = nullptr;
  a.y = part.data_ptr<float>();
  fill_conv_geometry(a, (int)M, 1, 1, (int)(K / splits), 1, 1, (int)N, (int)N, 1, 1, 1, 0, M, (int)K, false);
  a.ldx = (int)K;
  a.zero = zero_buffer(part.device()).data_ptr();
  a.ksplit = (int)splits;
  a.kslice = (int)(K / splits);
  a.ysplit = (long)(M * N);
}

}  // namespace idunno
