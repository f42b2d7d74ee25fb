// fp32 (f32 MFMA) convs and FC, the Winograd conv, and the packed-row RGB stem convs.
#include "binding_util.h"

using namespace idunno;

static const half_t* hp(const torch::Tensor& t) { return reinterpret_cast<const half_t*>(t.data_ptr()); }

// fp32 (reference precision) conv: y = act(conv(x, w) + bias (+ res)), all f32.
//   x   : [B, H, W, C] f32 NHWC, C == 4 (RGB+0 stem) or C % 16 == 0
//   w   : [Cout, Kpad] f32: big (kh, kw, c), Kpad = KH*KW*C;
//         small (kh, tap, c4) with taps padded to ceil(KW/4)*4, Kpad = KH*ceil(KW/4)*16
torch::Tensor conv2d_nhwc_f32(torch::Tensor x, torch::Tensor w, torch::Tensor bias, c10::optional<torch::Tensor> res,
                              int64_t KH, int64_t KW, int64_t stride, int64_t pad, bool relu, int64_t tile,
                              c10::optional<torch::Tensor> out) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kFloat, 4, dev);
  check_operand(w, "w", torch::kFloat, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  TORCH_CHECK(KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0, "bad conv geometry");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Cout = w.size(0), Kpad = w.size(1);
  TORCH_CHECK(bias.size(0) == Cout, "bias/Cout mismatch");
  TORCH_CHECK(Cout % 4 == 0, "Cout must be a multiple of 4");
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty output");
  const bool small = (C == 4);
  ConvF32Args a{};
  if (small) {
    a.nsub = (KW + 3) / 4;
    TORCH_CHECK(Kpad == KH * a.nsub * 16, "small-C f32 weight must be [Cout, KH*ceil(KW/4)*16]");
  } else {
    TORCH_CHECK(C % 16 == 0, "C must be 4 or a multiple of 16, got ", C);
    TORCH_CHECK(Kpad == KH * KW * C, "weight must be [Cout, KH*KW*C]");
    a.nsub = 1;
  }
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(M < (1L << 31) && (long)B * H * W * C < (1L << 31) && M * Cout < (1L << 40),
              "tensor too large for int32 indexing");
  auto y = optional_out(out, dev, torch::kFloat, {B, Ho, Wo, Cout});
  a.x = x.data_ptr<float>();
  a.w = w.data_ptr<float>();
  a.bias = bias.data_ptr<float>();
  a.res = static_cast<const float*>(optional_res(res, dev, torch::kFloat, {B, Ho, Wo, Cout}));
  a.y = y.data_ptr<float>();
  fill_conv_geometry(a, B, H, W, C, Ho, Wo, Cout, Cout, KH, KW, stride, pad, M, Kpad, relu);
  if (M == 0) return y;
  a.zero = zero_buffer(dev).data_ptr();
  const int t = tile >= 0 ? (int)tile : conv_f32_pick(a.M, Cout, Kpad, small);
  TORCH_CHECK(conv_f32_launch(a, small ? 1 : 0, t, cur_stream()), "unknown / unsupported f32 conv tile id ", t);
  check_launch("conv_f32");
  return y;
}

// fp32 FC layer y = act(x @ w.T + bias) with K split over `splits` slices in ONE
// conv_f32 launch (grid = tiles x splits, fp32 partials) + the split-K combine.
torch::Tensor linear_f32_splitk(torch::Tensor x, torch::Tensor w, torch::Tensor bias, bool relu, int64_t splits,
                                int64_t tile) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kFloat, 2, dev);
  check_operand(w, "w", torch::kFloat, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && bias.size(0) == N, "shape mismatch");
  TORCH_CHECK(N % 4 == 0, "N must be a multiple of 4");
  TORCH_CHECK(splits >= 1 && splits <= 16 && K % (16 * splits) == 0, "K must split into multiples of 16");
  TORCH_CHECK(splits * M * N < (1L << 31) && M * K < (1L << 31), "too large for int32 indexing");
  auto y = torch::empty({M, N}, x.options());
  if (M == 0) return y;
  auto part = torch::empty({splits, M, N}, x.options());
  const int64_t Ks = K / splits;
  ConvF32Args a{};
  a.x = x.data_ptr<float>();
  a.w = w.data_ptr<float>();
  fill_linear_splitk(a, M, K, N, splits, zero_f32(dev, N), part);
  const int t = tile >= 0 ? (int)tile : conv_f32_pick((int)M, (int)N, (int)Ks, false);
  TORCH_CHECK(t != 101 || Ks % 32 == 0, "tile 101 needs K slices of 32");
  TORCH_CHECK(conv_f32_launch(a, 0, t, cur_stream()), "unknown / unsupported f32 conv tile id ", t);
  check_launch("linear_f32_splitk");
  splitk_reduce_launch(part.data_ptr<float>(), (int)splits, (long)(M * N), (int)N, bias.data_ptr<float>(),
                       relu ? 1 : 0, y.data_ptr(), true, cur_stream());
  check_launch("splitk_reduce");
  return y;
}

// The checks and geometry the two packed-row stem convs share: x3 [B, H, copies * nc, wp]
// of dtype `dt` from preprocess_pack3*, w [Cout, .] of the same dtype, bias [Cout] f32.
struct Pack3 {
  int nc, wp, cpk, B, H, Cout, Kpad, Ho, Wo;
  long M;
};
static Pack3 pack3_checks(const torch::Tensor& x3, const torch::Tensor& w, const torch::Tensor& bias, int64_t W,
                          int64_t KH, int64_t KW, int64_t stride, int64_t pad, at::ScalarType dt, int copies,
                          const char* source) {
  const auto dev = x3.device();
  check_operand(x3, "x3", dt, 4, dev);
  check_operand(w, "w", dt, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  TORCH_CHECK(KH >= 1 && KW >= 5 && stride >= 1 && pad >= 0 && W >= 1, "pack3 stem geometry: KW >= 5");
  Pack3 p;
  pack3_geometry((int)W, (int)KW, (int)stride, (int)pad, dt == torch::kFloat ? 4 : 2, p.nc, p.wp, p.cpk);
  TORCH_CHECK(p.nc <= 4, "pack3 stem: stride needs at most 4 row copies");
  p.B = x3.size(0);
  p.H = x3.size(1);
  TORCH_CHECK(x3.size(2) == copies * p.nc && x3.size(3) == p.wp, "x3 must be [B, H, ", copies * p.nc, ", ", p.wp,
              "] (", source, ")");
  p.Cout = w.size(0);
  p.Kpad = w.size(1);
  TORCH_CHECK(bias.size(0) == p.Cout, "bias/Cout mismatch");
  p.Ho = (p.H + 2 * pad - KH) / stride + 1;
  p.Wo = ((int)W + 2 * pad - KW) / stride + 1;
  TORCH_CHECK(p.Ho > 0 && p.Wo > 0, "empty output");
  p.M = (long)p.B * p.Ho * p.Wo;
  TORCH_CHECK(p.M < (1L << 31) && (long)p.B * p.H * copies * p.nc * p.wp < (1L << 31),
              "tensor too large for int32 indexing");
  return p;
}

// RGB stem conv on packed rows: x3 [B, H, nc, wp] from preprocess_pack3 (fp32:
// conv_f32 mode 2 on the f32 MFMA; fp16: conv_glds pack3 on the f16 MFMA),
// w [Cout, nK * stage elements] (models/packed.py pack_conv_weight_p3), W = image width.
torch::Tensor conv2d_pack3(torch::Tensor x3, torch::Tensor w, torch::Tensor bias, int64_t W, int64_t KH,
                           int64_t KW, int64_t stride, int64_t pad, bool relu, int64_t tile) {
  const bool f16 = x3.scalar_type() == torch::kHalf;
  TORCH_CHECK(f16 || x3.scalar_type() == torch::kFloat, "x3 must be fp32 or fp16");
  const Pack3 p = pack3_checks(x3, w, bias, W, KH, KW, stride, pad, x3.scalar_type(), 1, "preprocess_pack3");
  // K stage = 16 fp32 / 64 fp16 elements = 4 / 8 chunks
  const int cps = f16 ? 8 : 4, nK = (KH * p.cpk + cps - 1) / cps;
  TORCH_CHECK(p.Kpad == nK * cps * (f16 ? 8 : 4), "pack3 weight must be [Cout, ", nK * cps * (f16 ? 8 : 4), "]");
  TORCH_CHECK(p.Cout % 4 == 0, "Cout must be a multiple of 4");
  auto y = torch::empty({p.B, p.Ho, p.Wo, p.Cout}, x3.options());
  if (p.M == 0) return y;
  const void* zero = zero_buffer(x3.device()).data_ptr();
  if (f16) {
    ConvArgs a{};
    a.x = hp(x3);
    a.w = hp(w);
    a.bias = bias.data_ptr<float>();
    a.y = y.data_ptr();
    fill_conv_geometry(a, p.B, p.H, (int)W, 3, p.Ho, p.Wo, p.Cout, p.Cout, KH, KW, stride, pad, p.M, p.Kpad, relu);
    a.nc = p.nc; a.wp = p.wp; a.cpk = p.cpk;
    a.zero = zero;
    const int t = tile >= 0 ? (int)tile : 27;
    TORCH_CHECK(conv_glds_launch(a, false, t, cur_stream()), "unsupported fp16 pack3 tile id ", t);
    check_launch("conv_glds_pack3");
    return y;
  }
  ConvF32Args a{};
  a.x = x3.data_ptr<float>();
  a.w = w.data_ptr<float>();
  a.bias = bias.data_ptr<float>();
  a.y = y.data_ptr<float>();
  fill_conv_geometry(a, p.B, p.H, (int)W, 3, p.Ho, p.Wo, p.Cout, p.Cout, KH, KW, stride, pad, p.M, p.Kpad, relu);
  a.nc = p.nc; a.wp = p.wp; a.cpk = p.cpk;
  a.zero = zero;
  const int t = tile >= 0 ? (int)tile : conv_f32_pick(a.M, p.Cout, p.Kpad, true);
  TORCH_CHECK(conv_f32_launch(a, 2, t, cur_stream()), "unknown / unsupported f32 conv tile id ", t);
  check_launch("conv_f32_pack3");
  return y;
}

// split-fp16 RGB stem on packed rows: x3 [B, H, 2*nc, wp] half (preprocess_pack3_split:
// nc hi copies, then nc lo copies), w [Cout, nK * 64] half (models/packed.py
// pack_split_weight_p3: per stage 32 K elements as [hi x32][lo x32]); fp32 output.
torch::Tensor conv2d_pack3_split(torch::Tensor x3, torch::Tensor w, torch::Tensor bias, int64_t W, int64_t KH,
                                 int64_t KW, int64_t stride, int64_t pad, bool relu, double acc_scale, int64_t tile) {
  const Pack3 p = pack3_checks(x3, w, bias, W, KH, KW, stride, pad, torch::kHalf, 2, "preprocess_pack3_split");
  const int nK = (KH * p.cpk + 3) / 4;                 // 4 input chunks (32 halfs) per split stage
  TORCH_CHECK(p.Kpad == nK * 64, "split pack3 weight must be [Cout, ", nK * 64, "]");
  TORCH_CHECK(p.Cout % 64 == 0 && p.M * p.Cout < (1L << 31), "Cout % 64, or tensor too large for int32 indexing");
  auto y = torch::empty({p.B, p.Ho, p.Wo, p.Cout}, x3.options().dtype(torch::kFloat));
  if (p.M == 0) return y;
  ConvArgs a{};
  a.x = hp(x3);
  a.w = hp(w);
  a.bias = bias.data_ptr<float>();
  a.y = y.data_ptr();
  fill_conv_geometry(a, p.B, p.H, (int)W, 3, p.Ho, p.Wo, p.Cout, p.Cout, KH, KW, stride, pad, p.M, p.Kpad, relu);
  a.acc_scale = (float)acc_scale;
  a.nc = p.nc; a.wp = p.wp; a.cpk = p.cpk;
  a.zero = zero_buffer(x3.device()).data_ptr();
  const int t = tile >= 0 ? (int)tile : 27;
  TORCH_CHECK(conv_glds_split_p3_launch(a, t, cur_stream()), "unsupported split pack3 tile id ", t);
  check_launch("conv_glds_split_pack3");
  return y;
}

// fp32 Winograd F(2x2,3x3) conv (3x3 / stride 1 / pad 1): x [B,H,W,C] f32 NHWC,
// u [16, Cout, C] f32 (= G g G^T, models/packed.py wino_weight), y = act(conv + bias (+ res)).
torch::Tensor conv2d_wino_f32(torch::Tensor x, torch::Tensor u, torch::Tensor bias, c10::optional<torch::Tensor> res,
                              bool relu, int64_t variant) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kFloat, 4, dev);
  check_operand(u, "u", torch::kFloat, 3, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  TORCH_CHECK(u.size(0) == 16, "U must be [16, Cout, C]");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Cout = u.size(1);
  TORCH_CHECK(u.size(2) == C && bias.size(0) == Cout, "U / bias shape mismatch");
  TORCH_CHECK(C % 16 == 0 && Cout % 32 == 0, "winograd conv needs C % 16 == 0 and Cout % 32 == 0");
  TORCH_CHECK(conv_wino_f32_supported(H, W, C, Cout), "winograd conv: unsupported image size");
  TORCH_CHECK((long)B * H * W * std::max(C, Cout) < (1L << 31), "tensor too large for int32 indexing");
  auto y = torch::empty({B, H, W, Cout}, x.options());
  WinoArgs a{};
  a.res = static_cast<const float*>(optional_res(res, dev, torch::kFloat, {B, H, W, Cout}));
  if (B == 0) return y;
  a.x = x.data_ptr<float>();
  a.u = u.data_ptr<float>();
  a.bias = bias.data_ptr<float>();
  a.y = y.data_ptr<float>();
  a.zero = zero_buffer(dev).data_ptr();
  a.B = B; a.H = H; a.W = W; a.C = C; a.Cout = Cout;
  a.relu = relu ? 1 : 0;
  a.ablate = 0;
  TORCH_CHECK(conv_wino_f32_launch(a, (int)variant, cur_stream()), "winograd conv launch rejected the shape");
  check_launch("conv_wino_f32");
  return y;
}
