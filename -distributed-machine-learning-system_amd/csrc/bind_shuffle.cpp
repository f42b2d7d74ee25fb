// ShuffleNetV2: the fused unit (split, 1x1, depthwise 3x3, 1x1, concat, channel shuffle), fp16 or fp32 by x's dtype.
#include "binding_util.h"
#include "shuffle_math.h"

using namespace idunno;

static bool fits(int64_t v) { return v > 0 && v < (1 << 24); }

static void check_mat(const torch::Tensor& t, const char* name, int64_t r, int64_t c) {
  TORCH_CHECK(t.size(0) == r && t.size(1) == c, name, ": must be [", r, ", ", c, "], got [", t.size(0), ", ", t.size(1),
              "]");
}
static void check_vec(const torch::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.size(0) == n, name, ": must have ", n, " elements, got ", t.size(0));
}

// out[B, Ho, Wo, Cp] = shuffle2(cat(left, right)), Cp = roundup(c, 8), pad channels zero
//   x      : [B, H, W, Cpin] half or float; stride 1: Cpin == Cp, left = x[..., :h], right reads x[..., h:c]
//   w1     : [hp, Kx] in x's dtype, b1 [hp] float       (hp, Kx: shuffle_math.h dims, ops.shuffle_plan)
//   wd     : [9, hp] in x's dtype tap-major, bd [hp] float
//   w2     : [hp, hp] in x's dtype, b2 [hp] float
//   stride 2 also: wd1 [9, Kx], bd1 [Kx] float, wp1 [hp, Kx], bp1 [hp] float (branch 1), and c is required
torch::Tensor shuffle_unit(torch::Tensor x, torch::Tensor w1, torch::Tensor b1, torch::Tensor wd, torch::Tensor bd,
                           torch::Tensor w2, torch::Tensor b2, int64_t stride, c10::optional<torch::Tensor> wd1,
                           c10::optional<torch::Tensor> bd1, c10::optional<torch::Tensor> wp1,
                           c10::optional<torch::Tensor> bp1, int64_t c, c10::optional<torch::Tensor> out) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2, got ", stride);
  check_operand(x, "x", dt, 4, dev);
  check_operand(w1, "w1", dt, 2, dev);
  check_operand(wd, "wd", dt, 2, dev);
  check_operand(w2, "w2", dt, 2, dev);
  check_operand(b1, "b1", torch::kFloat, 1, dev);
  check_operand(bd, "bd", torch::kFloat, 1, dev);
  check_operand(b2, "b2", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cpin = x.size(3);
  if (c < 0) {
    TORCH_CHECK(stride == 1, "c: the output width is required at stride 2");
    c = Cpin;
  }
  TORCH_CHECK(fits(H) && fits(W) && fits(Cpin) && Cpin % 8 == 0, "x: bad image size or channels not a multiple of 8");
  TORCH_CHECK(c > 0 && c % 2 == 0 && c <= shuffle::kMaxC, "c: must be even and at most ", shuffle::kMaxC, ", got ", c);
  // the logical input width only sets Cpin: any cin with roundup(cin, 8) == Cpin plans alike
  const int64_t cin = stride == 1 ? c : Cpin;
  shuffle::Plan p;
  TORCH_CHECK(shuffle::plan((int)H, (int)W, (int)cin, (int)c, (int)stride, f32, p), "shuffle_unit: no plan for H ", H,
              ", W ", W, ", c ", c, ", stride ", stride);
  TORCH_CHECK(p.cpin == Cpin, "x: must have ", p.cpin, " channels for c = ", c, " at stride ", stride, ", got ", Cpin);
  check_mat(w1, "w1", p.hp, p.Kx);
  check_mat(wd, "wd", 9, p.hp);
  check_mat(w2, "w2", p.hp, p.hp);
  check_vec(b1, "b1", p.hp);
  check_vec(bd, "bd", p.hp);
  check_vec(b2, "b2", p.hp);
  ShuffleUnitWeights w{};
  w.w1 = w1.data_ptr(); w.b1 = b1.data_ptr<float>();
  w.wd = wd.data_ptr(); w.bd = bd.data_ptr<float>();
  w.w2 = w2.data_ptr(); w.b2 = b2.data_ptr<float>();
  if (stride == 2) {
    TORCH_CHECK(wd1 && bd1 && wp1 && bp1, "stride 2 needs branch 1's operands wd1, bd1, wp1 and bp1");
    check_operand(*wd1, "wd1", dt, 2, dev);
    check_operand(*wp1, "wp1", dt, 2, dev);
    check_operand(*bd1, "bd1", torch::kFloat, 1, dev);
    check_operand(*bp1, "bp1", torch::kFloat, 1, dev);
    check_mat(*wd1, "wd1", 9, p.Kx);
    check_mat(*wp1, "wp1", p.hp, p.Kx);
    check_vec(*bd1, "bd1", p.Kx);
    check_vec(*bp1, "bp1", p.hp);
    w.wd1 = wd1->data_ptr(); w.bd1 = bd1->data_ptr<float>();
    w.wp1 = wp1->data_ptr(); w.bp1 = bp1->data_ptr<float>();
  } else {
    TORCH_CHECK(!wd1 && !bd1 && !wp1 && !bp1, "stride 1 takes no branch-1 operands");
  }
  TORCH_CHECK(B * H * W * std::max<int64_t>(Cpin, p.cp) < (1L << 31), "x: tensor too large for int32 indexing");
  auto y = optional_out(out, dev, dt, {B, (int64_t)p.Ho, (int64_t)p.Wo, (int64_t)p.cp});
  if (B == 0) return y;
  TORCH_CHECK(shuffle_unit_launch(x.data_ptr(), y.data_ptr(), w, (int)B, (int)H, (int)W, (int)cin, (int)c, (int)stride,
                                  f32, cur_stream()),
              "shuffle_unit: unsupported shape");
  check_launch(f32 ? "shuffle_unit_f32" : "shuffle_unit");
  return y;
}

// (R, bands, images a workgroup, LDS bytes, hp, Kx, Cp, Cpin, whole-image LDS bytes) of a unit shape; host only.  Raises where nothing plans.
std::vector<int64_t> shuffle_plan_py(int64_t H, int64_t W, int64_t cin, int64_t c, int64_t stride, bool f32) {
  int out[9];
  TORCH_CHECK(fits(H) && fits(W) && fits(cin) && fits(c) && (stride == 1 || stride == 2) &&
                  shuffle_plan((int)H, (int)W, (int)cin, (int)c, (int)stride, f32, out),
              "shuffle_plan: no plan for H ", H, ", W ", W, ", cin ", cin, ", c ", c, ", stride ", stride);
  return std::vector<int64_t>(out, out + 9);
}

bool shuffle_unit_ok_py(int64_t H, int64_t W, int64_t cin, int64_t c, int64_t stride) {
  if (!(fits(H) && fits(W) && fits(cin) && fits(c)) || (stride != 1 && stride != 2)) return false;
  int out[9];
  return shuffle_plan((int)H, (int)W, (int)cin, (int)c, (int)stride, false, out) &&
         shuffle_plan((int)H, (int)W, (int)cin, (int)c, (int)stride, true, out);
}
