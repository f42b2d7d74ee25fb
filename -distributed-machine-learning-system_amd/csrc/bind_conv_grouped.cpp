// grouped 3x3 conv (ResNeXt bottleneck middle conv): the fp16 and the split-fp16 form.
#include "binding_util.h"
#include "grouped_math.h"

using namespace idunno;

static const half_t* hp(const torch::Tensor& t) { return reinterpret_cast<const half_t*>(t.data_ptr()); }

// y = act(acc_scale * conv3x3(x, w; groups, stride, pad 1) + bias)
//   x : [B, H, W, C] half, or split [B, H, W, 2C]          C % 32 == 0, Cg = C / groups in {4, 8, 16, 32, 64}
//   w : [C, 9 CB] half (models/packed.py pack_grouped_weight), split: [C, 2 * 9 CB] (pack_grouped_split_weight)
//   y : [B, Ho, Wo, C] half, split: [B, Ho, Wo, 2C] (range-guarded)
static torch::Tensor grouped_impl(torch::Tensor x, torch::Tensor w, torch::Tensor bias, int64_t groups, int64_t stride,
                                  bool relu, bool split, double acc_scale) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), width = split ? 2 : 1, C = x.size(3) / width;
  TORCH_CHECK(C > 0 && x.size(3) == width * C && C % 32 == 0, "x: ", split ? "split input needs 2C halfs with " : "",
              "C % 32 == 0, got a last dim of ", x.size(3));
  TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2, got ", stride);
  TORCH_CHECK(groups > 1 && C % groups == 0, "groups: ", groups, " must be > 1 and divide x's C = ", C);
  const int64_t cg = C / groups;
  TORCH_CHECK(grouped::cg_ok((int)cg), "groups: C / groups = ", cg, " is not one of 4, 8, 16, 32, 64 (C ", C,
              ", groups ", groups, ")");
  const int64_t cb = grouped::block_of((int)cg);
  TORCH_CHECK(w.size(0) == C && w.size(1) == width * 9 * cb, "w: must be [C, ", width * 9 * cb, "] for C ", C,
              " and groups ", groups, ", got [", w.size(0), ", ", w.size(1), "]");
  TORCH_CHECK(bias.size(0) == C, "bias: must have C = ", C, " elements, got ", bias.size(0));
  const int64_t Ho = grouped::out_size((int)H, (int)stride), Wo = grouped::out_size((int)W, (int)stride);
  TORCH_CHECK(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "x: bad image size");
  TORCH_CHECK(B * H * W * width * C < (1L << 31) && B * Ho * Wo * width * C < (1L << 31),
              "x: tensor too large for int32 indexing");
  auto y = torch::empty({B, Ho, Wo, width * C}, x.options());
  if (B * Ho * Wo == 0) return y;
  TORCH_CHECK(conv3x3_grouped_launch(hp(x), hp(w), bias.data_ptr<float>(), reinterpret_cast<half_t*>(y.data_ptr()),
                                     (int)B, (int)H, (int)W, (int)C, (int)groups, (int)stride, relu ? 1 : 0, split,
                                     (float)acc_scale, split ? split_guard_for(dev) : nullptr, cur_stream()),
              "conv3x3_grouped: unsupported shape or too many tiles");
  check_launch(split ? "conv3x3_grouped_split" : "conv3x3_grouped");
  return y;
}

torch::Tensor conv3x3_grouped(torch::Tensor x, torch::Tensor w, torch::Tensor bias, int64_t groups, int64_t stride,
                              bool relu) {
  return grouped_impl(x, w, bias, groups, stride, relu, false, 1.0);
}

torch::Tensor conv3x3_grouped_split(torch::Tensor x, torch::Tensor w, torch::Tensor bias, double acc_scale,
                                    int64_t groups, int64_t stride, bool relu) {
  return grouped_impl(x, w, bias, groups, stride, relu, true, acc_scale);
}

bool conv3x3_grouped_ok(int64_t C, int64_t groups, int64_t stride) {
  return C > 0 && C < (1L << 31) && groups > 0 && groups < (1L << 31) &&
         conv3x3_grouped_supported((int)C, (int)groups, (int)stride);
}
