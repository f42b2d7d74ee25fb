// DenseNet: the fused dense layer on a concat buffer, the fused transition, the max pool into a wider buffer and the
// norm5 + ReLU + average pool head, fp16 or fp32 by the activation's dtype.
#include "binding_util.h"
#include "dense_math.h"

using namespace idunno;

static bool act_dtype(const torch::Tensor& t, const char* name) {
  const auto dt = t.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, name, " must be fp16 or fp32");
  return dt == torch::kFloat;
}

// buf[..., cin:cin + 32] = conv3x3 pad 1(relu(conv1x1(relu(buf[..., :cin] scale1 + shift1), w1) + b1), w2), in place
//   buf    : [B, H, W, Ctot] half or float, Ctot % 8 == 0, W <= 64
//   cin    : % 32 == 0, cin + 32 <= Ctot
//   scale1, shift1 : [cin] float (norm1 as an affine)
//   w1     : [128, cin] in buf's dtype (conv1 with norm2 folded in), b1 [128] float (norm2's shift)
//   w2     : [32, 9 * 128] in buf's dtype, tap-major
torch::Tensor dense_layer(torch::Tensor buf, int64_t cin, torch::Tensor scale1, torch::Tensor shift1, torch::Tensor w1,
                          torch::Tensor b1, torch::Tensor w2) {
  const bool f32 = act_dtype(buf, "buf");
  const auto dev = buf.device();
  const auto dt = buf.scalar_type();
  check_operand(buf, "buf", dt, 4, dev);
  check_operand(scale1, "scale1", torch::kFloat, 1, dev);
  check_operand(shift1, "shift1", torch::kFloat, 1, dev);
  check_operand(w1, "w1", dt, 2, dev);
  check_operand(b1, "b1", torch::kFloat, 1, dev);
  check_operand(w2, "w2", dt, 2, dev);
  const int64_t B = buf.size(0), H = buf.size(1), W = buf.size(2), Ctot = buf.size(3);
  TORCH_CHECK(cin > 0 && cin % 32 == 0 && cin <= dense::kMaxCin, "cin: must be a multiple of 32 up to ", dense::kMaxCin,
              ", got ", cin);
  TORCH_CHECK(cin + dense::kG <= Ctot, "cin: cin + 32 must be at most Ctot = ", Ctot, ", got cin = ", cin);
  TORCH_CHECK(Ctot % 8 == 0, "buf: Ctot must be a multiple of 8, got ", Ctot);
  TORCH_CHECK(H > 0 && W > 0, "buf: bad image size");
  TORCH_CHECK(W <= dense::kMaxW, "buf: W must be at most ", dense::kMaxW, ", got ", W);
  TORCH_CHECK(scale1.size(0) == cin, "scale1: must have cin = ", cin, " elements, got ", scale1.size(0));
  TORCH_CHECK(shift1.size(0) == cin, "shift1: must have cin = ", cin, " elements, got ", shift1.size(0));
  TORCH_CHECK(w1.size(0) == dense::kM && w1.size(1) == cin, "w1: must be [128, ", cin, "], got [", w1.size(0), ", ",
              w1.size(1), "]");
  TORCH_CHECK(b1.size(0) == dense::kM, "b1: must have 128 elements, got ", b1.size(0));
  TORCH_CHECK(w2.size(0) == dense::kG && w2.size(1) == 9 * dense::kM, "w2: must be [32, 1152], got [", w2.size(0), ", ",
              w2.size(1), "]");
  TORCH_CHECK(B * H * W * Ctot < (1L << 31), "buf: tensor too large for int32 indexing");
  if (B == 0) return buf;
  TORCH_CHECK(dense_layer_launch(buf.data_ptr(), scale1.data_ptr<float>(), shift1.data_ptr<float>(), w1.data_ptr(),
                                 b1.data_ptr<float>(), w2.data_ptr(), (int)B, (int)H, (int)W, (int)cin, (int)Ctot, f32,
                                 cur_stream()),
              "dense_layer: unsupported shape");
  check_launch(f32 ? "dense_layer_f32" : "dense_layer");
  return buf;
}

static bool fits(int64_t v) { return v > 0 && v < (1 << 24); }

bool dense_layer_ok_py(int64_t H, int64_t W, int64_t cin, int64_t Ctot) {
  if (!(fits(H) && fits(W) && fits(cin) && fits(Ctot))) return false;
  return dense_layer_ok((int)H, (int)W, (int)cin, (int)Ctot, false) &&
         dense_layer_ok((int)H, (int)W, (int)cin, (int)Ctot, true);
}

// (R, bands, mf, K chunk, x chunk bytes, LDS bytes) of a layer shape; host only.  Raises where nothing plans.
std::vector<int64_t> dense_plan_py(int64_t H, int64_t W, int64_t cin, bool f32) {
  int out[6];
  TORCH_CHECK(fits(H) && fits(W) && fits(cin) && dense_plan((int)H, (int)W, (int)cin, f32, out),
              "dense_plan: no plan for H ", H, ", W ", W, ", cin ", cin);
  return std::vector<int64_t>(out, out + 6);
}

// out[..., :C / 2] = conv1x1(avgpool2x2(relu(x scale + shift)), w)
//   x     : [B, H, W, C] half or float, C % 32 == 0, H, W >= 2 (odd sizes floor)
//   scale, shift : [C] float;  w : [C / 2, C] in x's dtype
//   out   : [B, H / 2, W / 2, Cnext] in x's dtype, Cnext % 8 == 0, Cnext >= C / 2; its other channels are untouched
torch::Tensor dense_transition(torch::Tensor x, torch::Tensor scale, torch::Tensor shift, torch::Tensor w,
                               torch::Tensor out) {
  const bool f32 = act_dtype(x, "buf");
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  check_operand(x, "buf", dt, 4, dev);
  check_operand(scale, "scale", torch::kFloat, 1, dev);
  check_operand(shift, "shift", torch::kFloat, 1, dev);
  check_operand(w, "w", dt, 2, dev);
  check_operand(out, "out", dt, 4, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), ldo = out.size(3);
  TORCH_CHECK(C > 0 && C % 32 == 0 && C <= dense::kMaxCin, "buf: C must be a multiple of 32 up to ", dense::kMaxCin,
              ", got ", C);
  TORCH_CHECK(H >= 2 && W >= 2, "buf: H and W must be at least 2");
  TORCH_CHECK(scale.size(0) == C, "scale: must have C = ", C, " elements, got ", scale.size(0));
  TORCH_CHECK(shift.size(0) == C, "shift: must have C = ", C, " elements, got ", shift.size(0));
  TORCH_CHECK(w.size(0) == C / 2 && w.size(1) == C, "w: must be [", C / 2, ", ", C, "], got [", w.size(0), ", ",
              w.size(1), "]");
  TORCH_CHECK(out.size(0) == B && out.size(1) == H / 2 && out.size(2) == W / 2, "out: must be [", B, ", ", H / 2, ", ",
              W / 2, ", >= ", C / 2, "]");
  TORCH_CHECK(ldo % 8 == 0 && ldo >= C / 2, "out: channels must be a multiple of 8 and at least C / 2 = ", C / 2,
              ", got ", ldo);
  TORCH_CHECK(B * H * W * C < (1L << 31) && out.numel() < (1L << 31), "buf: tensor too large for int32 indexing");
  if (B == 0) return out;
  TORCH_CHECK(dense_transition_launch(x.data_ptr(), scale.data_ptr<float>(), shift.data_ptr<float>(), w.data_ptr(),
                                      out.data_ptr(), (int)B, (int)H, (int)W, (int)C, (int)ldo, f32, cur_stream()),
              "dense_transition: unsupported shape");
  check_launch(f32 ? "dense_transition_f32" : "dense_transition");
  return out;
}

// buf[..., :C] = max pool k / s / pad of x; buf [B, Ho, Wo, Ctot] with Ctot >= C, its other channels untouched
torch::Tensor maxpool2d_into(torch::Tensor x, torch::Tensor buf, int64_t k, int64_t s, int64_t pad) {
  const bool f32 = act_dtype(x, "x");
  const auto dev = x.device();
  check_operand(x, "x", x.scalar_type(), 4, dev);
  check_operand(buf, "buf", x.scalar_type(), 4, dev);
  TORCH_CHECK(k >= 1 && s >= 1 && pad >= 0 && 2 * pad <= k && k < 64 && s < 64, "bad pool geometry");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), ldo = buf.size(3);
  TORCH_CHECK(H + 2 * pad >= k && W + 2 * pad >= k, "x: image smaller than the window");
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(C > 0 && C % 8 == 0, "x: C must be a multiple of 8, got ", C);
  TORCH_CHECK(buf.size(0) == B && buf.size(1) == Ho && buf.size(2) == Wo, "buf: must be [", B, ", ", Ho, ", ", Wo,
              ", >= ", C, "]");
  TORCH_CHECK(ldo % 8 == 0 && ldo >= C, "buf: channels must be a multiple of 8 and at least C = ", C, ", got ", ldo);
  TORCH_CHECK(x.numel() < (1L << 31) && buf.numel() < (1L << 31), "x: tensor too large for int32 indexing");
  if (B == 0) return buf;
  TORCH_CHECK(maxpool_into_launch(x.data_ptr(), buf.data_ptr(), (int)B, (int)H, (int)W, (int)C, (int)Ho, (int)Wo,
                                  (int)ldo, (int)k, (int)s, (int)pad, f32, cur_stream()),
              "maxpool2d_into: unsupported shape");
  check_launch(f32 ? "maxpool_into_f32" : "maxpool_into");
  return buf;
}

// [B, C] in buf's dtype = mean over pixels of relu(buf scale + shift); buf [B, H, W, C], C % 8 == 0
torch::Tensor bn_relu_avgpool(torch::Tensor buf, torch::Tensor scale, torch::Tensor shift) {
  const bool f32 = act_dtype(buf, "buf");
  const auto dev = buf.device();
  check_operand(buf, "buf", buf.scalar_type(), 4, dev);
  check_operand(scale, "scale", torch::kFloat, 1, dev);
  check_operand(shift, "shift", torch::kFloat, 1, dev);
  const int64_t B = buf.size(0), HW = buf.size(1) * buf.size(2), C = buf.size(3);
  TORCH_CHECK(C > 0 && C % 8 == 0, "buf: C must be a multiple of 8, got ", C);
  TORCH_CHECK(HW > 0 && HW < (1 << 24), "buf: bad image size");
  TORCH_CHECK(scale.size(0) == C, "scale: must have C = ", C, " elements, got ", scale.size(0));
  TORCH_CHECK(shift.size(0) == C, "shift: must have C = ", C, " elements, got ", shift.size(0));
  TORCH_CHECK(buf.numel() < (1L << 31), "buf: tensor too large for int32 indexing");
  auto y = torch::empty({B, C}, buf.options());
  if (B == 0) return y;
  TORCH_CHECK(bn_relu_avgpool_launch(buf.data_ptr(), scale.data_ptr<float>(), shift.data_ptr<float>(), y.data_ptr(),
                                     (int)B, (int)HW, (int)C, f32, cur_stream()),
              "bn_relu_avgpool: unsupported shape");
  check_launch(f32 ? "bn_relu_avgpool_f32" : "bn_relu_avgpool");
  return y;
}
