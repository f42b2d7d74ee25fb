// SqueezeNet: the fused Fire module and the pooled classifier head, fp16 or fp32 by x's dtype.
#include "binding_util.h"

using namespace idunno;

// y = concat(relu(conv1x1(s, w1) + b1), relu(conv3x3 pad 1(s, w3) + b3)),  s = relu(conv1x1(x, ws) + bs)
//   x  : [B, H, W, Cin] half or float, Cin % 16 == 0, Cin <= 512, W <= fire_max_w()
//   ws : [S, Kp] in x's dtype, S 16 | 32 | 48 | 64, Kp = conv1x1_narrow_kpad(Cin) (pack_pw_weight)
//   bs : [S] float
//   we : [E1 + E3, fire_kpad(S)] in x's dtype (models/packed.py pack_fire_weights); E1, E3 % 16 == 0, <= 256
//   be : [E1 + E3] float: b1 then b3
torch::Tensor fire(torch::Tensor x, torch::Tensor ws, torch::Tensor bs, torch::Tensor we, torch::Tensor be, int64_t e1,
                   c10::optional<torch::Tensor> out) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(x, "x", dt, 4, dev);
  check_operand(ws, "ws", dt, 2, dev);
  check_operand(we, "we", dt, 2, dev);
  check_operand(bs, "bs", torch::kFloat, 1, dev);
  check_operand(be, "be", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3), S = ws.size(0), N = we.size(0);
  const int64_t E1 = e1, E3 = N - e1;
  TORCH_CHECK(Cin > 0 && Cin % 16 == 0 && Cin <= 512, "x: Cin must be a multiple of 16 and at most 512, got ", Cin);
  TORCH_CHECK(S == 16 || S == 32 || S == 48 || S == 64, "ws: S must be 16, 32, 48 or 64, got ", S);
  TORCH_CHECK(E1 > 0 && E1 % 16 == 0 && E1 <= 256, "e1: E1 must be a multiple of 16 and at most 256, got ", E1);
  TORCH_CHECK(E3 > 0 && E3 % 16 == 0 && E3 <= 256, "we: E3 = rows - e1 must be a multiple of 16 and at most 256, got ",
              E3);
  TORCH_CHECK(H > 0 && W > 0, "x: bad image size");
  TORCH_CHECK(W <= fire_max_w(), "x: W must be at most ", fire_max_w(), ", got ", W);
  const int64_t Kp = conv1x1_narrow_kpad((int)Cin, f32), KpE = fire_kpad((int)S, f32);
  TORCH_CHECK(ws.size(1) == Kp, "ws: must be [S, ", Kp, "] for Cin ", Cin, ", got [", S, ", ", ws.size(1), "]");
  TORCH_CHECK(we.size(1) == KpE, "we: must be [E1 + E3, ", KpE, "] for S ", S, ", got [", N, ", ", we.size(1), "]");
  TORCH_CHECK(bs.size(0) == S, "bs: must have S = ", S, " elements, got ", bs.size(0));
  TORCH_CHECK(be.size(0) == N, "be: must have E1 + E3 = ", N, " elements, got ", be.size(0));
  TORCH_CHECK(B * H * W * std::max(Cin, N) < (1L << 31), "x: tensor too large for int32 indexing");
  auto y = optional_out(out, dev, dt, {B, H, W, N});
  if (B == 0) return y;
  TORCH_CHECK(fire_launch(x.data_ptr(), ws.data_ptr(), bs.data_ptr<float>(), we.data_ptr(), be.data_ptr<float>(),
                          y.data_ptr(), (int)B, (int)H, (int)W, (int)Cin, (int)S, (int)E1, (int)E3, f32, cur_stream()),
              "fire: unsupported shape");
  check_launch(f32 ? "fire_f32" : "fire");
  return y;
}

bool fire_ok_py(int64_t H, int64_t W, int64_t Cin, int64_t S, int64_t E1, int64_t E3) {
  const auto fits = [](int64_t v) { return v > 0 && v < (1 << 24); };
  if (!(fits(H) && fits(W) && fits(Cin) && fits(S) && fits(E1) && fits(E3))) return false;
  return fire_ok((int)H, (int)W, (int)Cin, (int)S, (int)E1, (int)E3, false) &&
         fire_ok((int)H, (int)W, (int)Cin, (int)S, (int)E1, (int)E3, true);
}

// out[b, n] = mean over pixels of relu(x[b, p, :] . w[n, :] + bias[n]), fp32 [B, N]
//   x    : [B, H, W, K] half or float, K % 8 == 0, K <= 1280
//   w    : [N, Kp] in x's dtype (pack_pw_weight), N % 8 == 0, N <= 1280
//   bias : [N] float
torch::Tensor conv1x1_relu_pool(torch::Tensor x, torch::Tensor w, torch::Tensor bias) {
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kFloat, "x must be fp16 or fp32");
  const bool f32 = dt == torch::kFloat;
  check_operand(x, "x", dt, 4, dev);
  check_operand(w, "w", dt, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t B = x.size(0), HW = x.size(1) * x.size(2), K = x.size(3), N = w.size(0);
  TORCH_CHECK(K > 0 && K % 8 == 0 && K <= 1280, "x: K must be a multiple of 8 and at most 1280, got ", K);
  TORCH_CHECK(N > 0 && N % 8 == 0 && N <= 1280, "w: N must be a multiple of 8 and at most 1280, got ", N);
  const int64_t Kp = conv1x1_narrow_kpad((int)K, f32);
  TORCH_CHECK(w.size(1) == Kp, "w: must be [N, ", Kp, "] for K ", K, ", got [", N, ", ", w.size(1), "]");
  TORCH_CHECK(bias.size(0) == N, "bias: must have N = ", N, " elements, got ", bias.size(0));
  TORCH_CHECK(HW > 0 && B * HW * K < (1L << 31) && B < (1 << 24), "x: bad size or too large for int32 indexing");
  auto y = torch::empty({B, N}, x.options().dtype(torch::kFloat));
  if (B == 0) return y;
  TORCH_CHECK(conv1x1_pool_launch(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), y.data_ptr<float>(), (int)B,
                                  (int)HW, (int)K, (int)N, f32, cur_stream()),
              "conv1x1_relu_pool: unsupported shape");
  check_launch(f32 ? "conv1x1_pool_f32" : "conv1x1_pool");
  return y;
}
