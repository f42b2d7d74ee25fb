// depthwise 3x3 conv (MobileNetV2's middle conv), fp16 or fp32 by x's dtype.
#include "binding_util.h"

using namespace idunno;

// y = act(conv3x3 depthwise(x, w9; stride, pad 1) + bias)
//   x    : [B, H, W, C] half or float          C % 8 == 0 (float: % 4)
//   w9   : [9, C] in x's dtype, tap-major (models/packed.py pack_dw_weight)
//   bias : [C] float
//   act  : 0 none, 1 ReLU, 2 ReLU6;  clamp_in: min(x, 6) on every loaded input value
torch::Tensor conv3x3_dw(torch::Tensor x, torch::Tensor w9, torch::Tensor bias, int64_t stride, int64_t act,
                         bool clamp_in, c10::optional<torch::Tensor> out) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(x, "x", dt, 4, dev);
  check_operand(w9, "w9", dt, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), mult = f32 ? 4 : 8;
  TORCH_CHECK(C > 0 && C % mult == 0, "x: C must be a multiple of ", mult, ", got ", C);
  TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2, got ", stride);
  TORCH_CHECK(act >= 0 && act <= 2, "act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got ", act);
  TORCH_CHECK(w9.size(0) == 9 && w9.size(1) == C, "w9: must be [9, ", C, "], got [", w9.size(0), ", ", w9.size(1), "]");
  TORCH_CHECK(bias.size(0) == C, "bias: must have C = ", C, " elements, got ", bias.size(0));
  TORCH_CHECK(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "x: bad image size");
  TORCH_CHECK(B * H * W * C < (1L << 31), "x: tensor too large for int32 indexing");
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  auto y = optional_out(out, dev, dt, {B, Ho, Wo, C});
  if (B == 0) return y;
  TORCH_CHECK(conv3x3_dw_launch(x.data_ptr(), w9.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), (int)B, (int)H,
                                (int)W, (int)C, (int)stride, (int)act, clamp_in ? 1 : 0, f32, cur_stream()),
              "conv3x3_dw: unsupported shape");
  check_launch(f32 ? "conv3x3_dw_f32" : "conv3x3_dw");
  return y;
}
