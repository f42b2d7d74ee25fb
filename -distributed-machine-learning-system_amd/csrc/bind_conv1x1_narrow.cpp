// narrow-channel 1x1 conv (MobileNetV2 / V3's expand / project convs), fp16 or fp32 by x's dtype.
#include "binding_util.h"

using namespace idunno;

// y = act(conv1x1(in_scale * x, w) + bias (+ res_act(residual)))
//   x        : [B, H, W, K] half or float, K % 8 == 0, K <= 1280; a channel slice of a wider NHWC tensor is
//              read in place (contiguous channels, equally spaced 16-byte aligned pixels)
//   w        : [N, Kp] in x's dtype, Kp = K rounded up to 32 (float: 16), zero from K (pack_pw_weight)
//   bias     : [N] float, N % 8 == 0, N <= 1280
//   residual : [B, H, W, N] in x's dtype, contiguous, added before act; res_act 3: after its own hardswish
//   in_scale : [B, K] in x's dtype, contiguous: image b's pixels are multiplied by row b (rounded to x's dtype)
//   act      : 0 none, 1 ReLU, 2 ReLU6, 3 hardswish, 4 hardsigmoid
torch::Tensor conv1x1_narrow(torch::Tensor x, torch::Tensor w, torch::Tensor bias, int64_t act,
                             c10::optional<torch::Tensor> residual, c10::optional<torch::Tensor> out,
                             c10::optional<torch::Tensor> in_scale, int64_t res_act) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(x, "x", dt, 4, dev, false);
  check_operand(w, "w", dt, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), K = x.size(3), N = w.size(0), M = B * H * W;
  TORCH_CHECK(K > 0 && K % 8 == 0 && K <= 1280, "x: K must be a multiple of 8 and at most 1280, got ", K);
  const int64_t ldx = nhwc_pixel_stride(x, "x");
  TORCH_CHECK(N > 0 && N % 8 == 0 && N <= 1280, "w: N must be a multiple of 8 and at most 1280, got ", N);
  const int64_t Kp = conv1x1_narrow_kpad((int)K, f32);
  TORCH_CHECK(w.size(1) == Kp, "w: must be [N, ", Kp, "] for K ", K, ", got [", N, ", ", w.size(1), "]");
  TORCH_CHECK(bias.size(0) == N, "bias: must have N = ", N, " elements, got ", bias.size(0));
  TORCH_CHECK(act >= 0 && act <= 4, "act must be 0 (none), 1 (ReLU), 2 (ReLU6), 3 (hardswish) or 4 (hardsigmoid), got ",
              act);
  TORCH_CHECK(res_act == 0 || res_act == 3, "res_act must be 0 (none) or 3 (hardswish), got ", res_act);
  TORCH_CHECK(res_act == 0 || residual.has_value(), "res_act needs a residual");
  const void* sp = nullptr;
  if (in_scale.has_value()) {
    check_operand(*in_scale, "in_scale", dt, 2, dev);
    TORCH_CHECK(in_scale->size(0) == B && in_scale->size(1) == K, "in_scale: must be [", B, ", ", K, "], got [",
                in_scale->size(0), ", ", in_scale->size(1), "]");
    sp = in_scale->data_ptr();
  }
  TORCH_CHECK(M * ldx < (1L << 31) && M * N < (1L << 31), "x: tensor too large for int32 indexing");
  const void* rp = optional_res(residual, dev, dt, {B, H, W, N});
  auto y = optional_out(out, dev, dt, {B, H, W, N});
  if (M == 0) return y;
  TORCH_CHECK(conv1x1_narrow_launch(x.data_ptr(), (int)ldx, w.data_ptr(), bias.data_ptr<float>(), rp, y.data_ptr(),
                                    (int)M, (int)K, (int)N, (int)act, f32, cur_stream(), sp, (int)(H * W),
                                    (int)res_act),
              "conv1x1_narrow: unsupported shape");
  check_launch(f32 ? "conv1x1_narrow_f32" : "conv1x1_narrow");
  return y;
}
