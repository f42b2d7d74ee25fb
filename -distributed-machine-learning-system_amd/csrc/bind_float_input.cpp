// Normalised float images -> stem operands (kernels/float_input.hip): the float
// counterparts of preprocess / preprocess_pack3 / preprocess_pack3_split.
//
// x is fp32 or fp16 of logical shape [B, 3, H, W], read through its strides:
// NCHW (pixel stride 1; any plane, row and image strides) or channels-last
// (pixel stride 3, channel stride 1; any row and image strides), so a
// contiguous tensor, a torch.channels_last one and batch views of either
// (x[::2], x[1:]) are read in place.  No device-side window: float batches are
// not resident shards.
#include "binding_util.h"
#include "float_input_math.h"

using namespace idunno;

static torch::Tensor float_input(const torch::Tensor& x, FloatInForm form, int64_t KW, int64_t stride, int64_t pad) {
  const bool f16 = x.scalar_type() == torch::kHalf;
  TORCH_CHECK(f16 || x.scalar_type() == torch::kFloat, "x must be fp32 or fp16 (got ", x.scalar_type(), ")");
  check_operand(x, "x", x.scalar_type(), 4, x.device(), false);
  TORCH_CHECK(x.size(1) == 3, "x must be [B, 3, H, W] (got ", x.sizes(), ")");
  const int64_t B = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(B == 0 || (H >= 1 && W >= 1), "empty image");
  const bool cl = x.stride(3) == 3 && x.stride(1) == 1;
  TORCH_CHECK(cl || x.stride(3) == 1,
              "x must be NCHW (innermost stride 1) or channels-last (pixel stride 3, channel stride 1); strides ",
              x.strides());
  TORCH_CHECK(x.stride(0) >= 0 && x.stride(1) >= 0 && x.stride(2) >= 0, "x must not have negative strides");

  FloatInArgs a{};
  a.pad = 0; a.nc = 1; a.wp = 0;
  torch::Tensor out;
  if (form == kFiNhwc4F16 || form == kFiNhwc4F32) {
    TORCH_CHECK(B * H * W * 4 < (1L << 31), "tensor too large for int32 indexing");
    out = torch::empty({B, H, W, 4}, x.options().dtype(form == kFiNhwc4F32 ? torch::kFloat : torch::kHalf)
                                         .memory_format(torch::MemoryFormat::Contiguous));
  } else {
    TORCH_CHECK(KW >= 5 && stride >= 1 && pad >= 0, "pack3 stem geometry: KW >= 5");
    TORCH_CHECK(W < (1 << 24) && pad < (1 << 24), "image too wide");
    int cpk;
    pack3_geometry((int)W, (int)KW, (int)stride, (int)pad, form == kFiPack3F32 ? 4 : 2, a.nc, a.wp, cpk);
    TORCH_CHECK(a.nc <= 4, "pack3 stem: stride needs at most 4 row copies");
    const int copies = form == kFiPack3Split ? 2 : 1;
    TORCH_CHECK(B * H * copies * a.nc * a.wp < (1L << 31), "tensor too large for int32 indexing");
    out = torch::empty({B, H, copies * a.nc, a.wp},
                       x.options().dtype(form == kFiPack3F32 ? torch::kFloat : torch::kHalf)
                           .memory_format(torch::MemoryFormat::Contiguous));
    a.pad = (int)pad;
  }
  if (B == 0) return out;
  // the farthest source element, in elements from x's first
  const int64_t span = (B - 1) * x.stride(0) + 2 * x.stride(1) + (H - 1) * x.stride(2) + (W - 1) * x.stride(3);
  TORCH_CHECK(span < (1L << 31), "tensor too large for int32 indexing");
  a.rows = fi_band_rows((int)W);
  TORCH_CHECK(a.rows >= 1, "image too wide: a row of ", W, " pixels does not fit the LDS band");
  a.nbands = (int)((H + a.rows - 1) / a.rows);
  TORCH_CHECK(B * a.nbands < (1L << 31), "batch too large");
  a.src = x.data_ptr();
  a.out = out.data_ptr();
  a.sb = x.stride(0); a.sc = x.stride(1); a.sh = x.stride(2);
  a.B = (int)B; a.H = (int)H; a.W = (int)W;
  a.guard = form == kFiPack3Split ? split_guard_for(x.device()) : nullptr;
  float_input_launch(a, f16, cl, form, cur_stream());
  check_launch("float_input");
  return out;
}

// [B,3,H,W] float -> [B,H,W,4] fp16 (f32: fp32), 4th channel 0: what preprocess writes
torch::Tensor float_to_nhwc4(torch::Tensor x, bool f32) {
  return float_input(x, f32 ? kFiNhwc4F32 : kFiNhwc4F16, 0, 0, 0);
}

// -> packed rows [B, H, nc, wp] fp32 (f16: fp16) of a KW-wide stem: what preprocess_pack3 writes
torch::Tensor float_to_pack3(torch::Tensor x, int64_t KW, int64_t stride, int64_t pad, bool f16) {
  return float_input(x, f16 ? kFiPack3F16 : kFiPack3F32, KW, stride, pad);
}

// -> split packed rows [B, H, 2*nc, wp] fp16 (hi copies, lo copies): what preprocess_pack3_split
// writes; with the split guard armed a value outside fp16's range (or not finite) sets it
torch::Tensor float_to_pack3_split(torch::Tensor x, int64_t KW, int64_t stride, int64_t pad) {
  return float_input(x, kFiPack3Split, KW, stride, pad);
}
