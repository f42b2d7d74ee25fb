// depthwise convs (MobileNetV2 / V3's middle conv) and V3's squeeze-and-excitation gate, fp16 or fp32 by x's dtype.
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

// y = act(depthwise k x k conv(act_in(x), w; stride, pad k / 2) + bias), and with `pool` also its spatial mean
//   x      : [B, H, W, C] half or float          C % 8 == 0 (float: % 4)
//   w      : [k k, C] in x's dtype, tap-major (models/packed.py pack_dw_weight), k 3 or 5
//   bias   : [C] float
//   act    : 0 none, 1 ReLU, 2 ReLU6, 3 hardswish;  act_in: 0 none, 3 hardswish on every loaded input value
//   pool   : [B, C] in x's dtype, contiguous: receives mean over (Ho, Wo) of y as stored (no atomics)
torch::Tensor conv_dw(torch::Tensor x, torch::Tensor w, torch::Tensor bias, int64_t k, int64_t stride, int64_t act,
                      int64_t act_in, c10::optional<torch::Tensor> pool, c10::optional<torch::Tensor> out) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(x, "x", dt, 4, dev);
  check_operand(w, "w", dt, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), mult = f32 ? 4 : 8;
  TORCH_CHECK(C > 0 && C % mult == 0, "x: C must be a multiple of ", mult, ", got ", C);
  TORCH_CHECK(k == 3 || k == 5, "k must be 3 or 5, got ", k);
  TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2, got ", stride);
  TORCH_CHECK(act >= 0 && act <= 3, "act must be 0 (none), 1 (ReLU), 2 (ReLU6) or 3 (hardswish), got ", act);
  TORCH_CHECK(act_in == 0 || act_in == 3, "act_in must be 0 (none) or 3 (hardswish), got ", act_in);
  TORCH_CHECK(w.size(0) == k * k && w.size(1) == C, "w: must be [", k * k, ", ", C, "], got [", w.size(0), ", ",
              w.size(1), "]");
  TORCH_CHECK(bias.size(0) == C, "bias: must have C = ", C, " elements, got ", bias.size(0));
  TORCH_CHECK(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "x: bad image size");
  TORCH_CHECK(B * H * W * C < (1L << 31), "x: tensor too large for int32 indexing");
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  void* pp = nullptr;
  if (pool.has_value()) {
    check_operand(*pool, "pool", dt, 2, dev);
    TORCH_CHECK(pool->size(0) == B && pool->size(1) == C, "pool: must be [", B, ", ", C, "], got [", pool->size(0),
                ", ", pool->size(1), "]");
    TORCH_CHECK(conv_dw_pool_ok((int)Wo), "pool: an output width of ", Wo,
                " does not fit the pooled split (one workgroup per image: at most 256 columns)");
    pp = pool->data_ptr();
  }
  auto y = optional_out(out, dev, dt, {B, Ho, Wo, C});
  if (B == 0) return y;
  TORCH_CHECK(conv_dw_kxk_launch(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), pp, (int)B, (int)H,
                                 (int)W, (int)C, (int)k, (int)stride, (int)act, (int)act_in, f32, cur_stream()),
              "conv_dw: unsupported shape");
  check_launch(f32 ? "conv_dw_kxk_f32" : "conv_dw_kxk");
  return y;
}

// scale = hardsigmoid(w2 relu(w1 mean + b1) + b2)
//   mean   : [B, C] half or float, C % 8 == 0, C <= 1280
//   w1, w2 : [Csq, kpad(C)], [C, kpad(Csq)] in mean's dtype (pack_pw_weight), Csq % 8 == 0, Csq <= 320
//   b1, b2 : [Csq], [C] float
torch::Tensor se_excite(torch::Tensor mean, torch::Tensor w1, torch::Tensor b1, torch::Tensor w2, torch::Tensor b2) {
  const auto dev = mean.device();
  const auto dt = mean.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "mean must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(mean, "mean", dt, 2, dev);
  check_operand(w1, "w1", dt, 2, dev);
  check_operand(w2, "w2", dt, 2, dev);
  check_operand(b1, "b1", torch::kFloat, 1, dev);
  check_operand(b2, "b2", torch::kFloat, 1, dev);
  const int64_t B = mean.size(0), C = mean.size(1), Csq = w1.size(0);
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 1280, "mean: C must be a multiple of 8 and at most 1280, got ", C);
  TORCH_CHECK(Csq > 0 && Csq % 8 == 0 && Csq <= 320, "w1: Csq must be a multiple of 8 and at most 320, got ", Csq);
  const int64_t Kp1 = conv1x1_narrow_kpad((int)C, f32), Kp2 = conv1x1_narrow_kpad((int)Csq, f32);
  TORCH_CHECK(w1.size(1) == Kp1, "w1: must be [", Csq, ", ", Kp1, "], got [", Csq, ", ", w1.size(1), "]");
  TORCH_CHECK(w2.size(0) == C && w2.size(1) == Kp2, "w2: must be [", C, ", ", Kp2, "], got [", w2.size(0), ", ",
              w2.size(1), "]");
  TORCH_CHECK(b1.size(0) == Csq && b2.size(0) == C, "b1 / b2: must have ", Csq, " / ", C, " elements");
  TORCH_CHECK(B * C < (1L << 31), "mean: tensor too large for int32 indexing");
  auto scale = torch::empty({B, C}, mean.options());
  if (B == 0) return scale;
  TORCH_CHECK(se_excite_launch(mean.data_ptr(), w1.data_ptr(), b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), scale.data_ptr(), (int)B, (int)C, (int)Csq, f32, cur_stream()),
              "se_excite: unsupported shape");
  check_launch(f32 ? "se_excite_f32" : "se_excite");
  return scale;
}
