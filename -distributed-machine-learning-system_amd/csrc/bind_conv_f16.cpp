// fp16 convs and FC: conv2d_nhwc, the bottleneck 1x1 fusions, the band-staged 3x3, linear_splitk.
#include "binding_util.h"

using namespace idunno;

static const half_t* hp(const torch::Tensor& t) { return reinterpret_cast<const half_t*>(t.data_ptr()); }

// y = act(conv(x, w) + bias (+ res))
//   x   : [B, H, W, C] fp16 NHWC (C == 4 for the small-C stem path, else C % 64 == 0)
//   w   : [Cout, Kpad] fp16, K ordered (kh, kw, c) [big] or (kh, kw8, c4) [small]
//   bias: [Cout] fp32
//   res : optional [B, Ho, Wo, Cout] fp16
torch::Tensor conv2d_nhwc(torch::Tensor x, torch::Tensor w, torch::Tensor bias,
                          c10::optional<torch::Tensor> res, int64_t KH, int64_t KW, int64_t stride,
                          int64_t pad, bool relu, bool out_f32, int64_t tile, c10::optional<torch::Tensor> out,
                          int64_t ksplit, int64_t route) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  TORCH_CHECK(KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0, "bad conv geometry");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Cout = w.size(0), Kpad = w.size(1);
  TORCH_CHECK(bias.size(0) == Cout, "bias/Cout mismatch");
  TORCH_CHECK(Cout % 4 == 0, "Cout must be a multiple of 4");
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty output");
  const bool small = (C == 4);
  ConvArgs a{};
  if (small) {
    const int nsub = (KW + 7) / 8;
    TORCH_CHECK(Kpad == KH * nsub * 32, "small-C weight must be [Cout, KH*ceil(KW/8)*32]");
    a.nsub = nsub;
    a.nK = KH * nsub;
    a.cblk = 1;
  } else {
    TORCH_CHECK(C % 64 == 0, "C must be 4 or a multiple of 64, got ", C);
    TORCH_CHECK(Kpad == KH * KW * C, "weight must be [Cout, KH*KW*C]");
    a.cblk = C / 64;
    a.nK = KH * KW * a.cblk;
    a.nsub = 1;
  }
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(M < (1L << 31) && (long)B * H * W * C < (1L << 31), "tensor too large for int32 indexing");
  auto y = optional_out(out, dev, out_f32 ? torch::kFloat : torch::kHalf, {B, Ho, Wo, Cout});
  const half_t* rp = static_cast<const half_t*>(optional_res(res, dev, torch::kHalf, {B, Ho, Wo, Cout}));
  TORCH_CHECK(rp == nullptr || !out_f32 || !small, "unsupported combination");
  a.x = hp(x);
  a.w = hp(w);
  a.bias = bias.data_ptr<float>();
  a.res = rp;
  a.y = y.data_ptr();
  fill_conv_geometry(a, B, H, W, C, Ho, Wo, Cout, Cout, KH, KW, stride, pad, M, Kpad, relu);
  if (M == 0) return y;
  if (small) {
    const int t = (tile >= 0 && tile <= 3) ? (int)tile : conv_pick_tile(a.M, Cout);
    conv_igemm_launch(a, small, out_f32, t, cur_stream()); check_launch("conv_igemm");
    return y;
  }
  if (tile >= 0 && tile <= 3) {          // v1 register-staged loop (kept for A/B)
    conv_igemm_launch(a, small, out_f32, (int)tile, cur_stream()); check_launch("conv_igemm");
    return y;
  }
  a.zero = zero_buffer(dev).data_ptr();
  const bool c64_ok = KH == 3 && KW == 3 && stride == 1 && pad == 1 && !out_f32 && conv3x3_c64_supported(C, Cout);
  // resident-weight 3x3 64->64 kernel (tile 50, conv3x3_c64.hip): since sweep r1 #6 (ResNet18
  // layer1 at B=400: 112 / 153 us vs 178 / 207 us for the best im2col tile, profiles/r1_v6_layer1_c64.log)
  if (tile == 50 || (tile < 0 && c64_ok && !(route & kRouteNoC64))) {
    TORCH_CHECK(c64_ok, "tile 50 (resident-weight 3x3 64->64 conv) does not support this shape");
    conv3x3_c64_launch(a.x, a.w, a.bias, a.res, reinterpret_cast<half_t*>(a.y), a.zero, B, H, W, a.relu,
                       cur_stream()); check_launch("conv3x3_c64");
    return y;
  }
  // band-staged 3x3 kernel in fp16 (conv3x3_band.hip, tile 70): ResNet layers 2-4
  const bool band_ok = KH == 3 && KW == 3 && stride == 1 && pad == 1 && !out_f32 &&
                       conv3x3_band_supported(H, W, C, Cout);
  if (tile == 70 || (tile < 0 && band_ok && !(route & kRouteNoBand) && conv3x3_band_f16_default(B, W, Cout, rp != nullptr))) {
    TORCH_CHECK(band_ok, "tile 70 (band-staged 3x3 conv) does not support this shape");
    TORCH_CHECK(conv3x3_band_launch(a.x, C, a.w, a.bias, rp, Cout, a.y, Cout, false, B, H, W, C, Cout, a.relu, 1.0f,
                                    nullptr, 0, 0, cur_stream(), true),
                "band conv: tensor too large for 32-bit buffer offsets");
    check_launch("conv3x3_band (fp16)");
    return y;
  }
  const bool c1s_ok = KH == 1 && KW == 1 && (stride == 1 || stride == 2) && pad == 0 && !out_f32 &&
                      conv1x1_stream_supported(C, Cout, M);
  if (tile == 80 || (tile < 0 && c1s_ok && !(route & kRouteNoStream1x1) && conv1x1_stream_default(C, stride, M))) {
    TORCH_CHECK(c1s_ok, "tile 80 (streaming 1x1 conv) does not support this shape");
    conv1x1_stream_launch(a.x, a.w, a.bias, a.res, reinterpret_cast<half_t*>(a.y), a.zero, a.M, C, Cout, a.relu,
                          H, W, Wo, Ho * Wo, stride, cur_stream()); check_launch("conv1x1_stream");
    return y;
  }
  const int t = tile >= 10 ? (int)tile : conv_glds_pick(a.M, Cout);
  // split-K: auto only for the auto-picked tile (a forced tile runs its own epilogue)
  const int ks = C % 64 == 0 ? conv_f16_ksplit(a.M, Cout, t, (int)(KH * KW) * (C / 64),
                                               tile >= 0 && ksplit < 0 ? 1 : (int)ksplit) : 1;
  TORCH_CHECK(ksplit <= 1 || ks == ksplit, "split-K: ", ksplit, " slices do not divide the K loop of tile ", t);
  if (ks > 1) {
    // small M: K slices into fp32 partials, one combine (conv2d_split_impl, conv_glds.hip conv_split_ksplit)
    TORCH_CHECK((long)ks * M * Cout < (1L << 31), "split-K partials too large for int32 indexing");
    auto part = torch::empty({ks, M, (int64_t)Cout}, x.options().dtype(torch::kFloat));
    auto zb = zero_f32(dev, Cout);
    ConvArgs b = a;
    b.bias = zb.data_ptr<float>();
    b.res = nullptr;
    b.y = part.data_ptr<float>();
    b.ldy = Cout;
    b.relu = 0;
    b.ksplit = ks;
    b.kslice = 0;
    b.ysplit = (long)M * Cout;
    b.kstage = (int)(KH * KW) * (C / 64) / ks;
    TORCH_CHECK(conv_glds_launch(b, true, t, cur_stream()), "unknown conv tile id ", t);
    check_launch("conv_glds (split-K)");
    splitk_reduce_res_launch(part.data_ptr<float>(), ks, (long)M * Cout, Cout, a.bias, rp, Cout, a.relu, a.y, Cout,
                             out_f32 ? 3 : 2, nullptr, cur_stream());
    check_launch("splitk_reduce_res");
    return y;
  }
  TORCH_CHECK(conv_glds_launch(a, out_f32, t, cur_stream()), "unknown conv tile id ", t);
  check_launch("conv_glds");
  return y;
}

// ResNet bottleneck tail as ONE GEMM: y = act([x1 | x2 gathered at stride] .
// [W3 | Wds]^T + b), i.e. the expansion 1x1 conv of the block's last conv
// input x1 plus the 1x1 (strided) downsample of the block input x2, whose sum
// is the residual add -- the downsample's output never reaches HBM
// (conv1x1_stream.hip, dual input).
//   x1 [B, Ho, Wo, K1] fp16, x2 [B, H, W, K2] fp16, w [Cout, K1 + K2] fp16, bias [Cout] f32
torch::Tensor conv1x1_dual(torch::Tensor x1, torch::Tensor x2, torch::Tensor w, torch::Tensor bias, int64_t stride,
                           bool relu) {
  const auto dev = x1.device();
  check_operand(x1, "x1", torch::kHalf, 4, dev);
  check_operand(x2, "x2", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int B = x1.size(0), Ho = x1.size(1), Wo = x1.size(2), K1 = x1.size(3);
  const int H = x2.size(1), W = x2.size(2), K2 = x2.size(3);
  const int Cout = w.size(0);
  check_strided_input(x2, B, Ho, Wo, stride);
  TORCH_CHECK(w.size(1) == K1 + K2 && bias.size(0) == Cout, "weight must be [Cout, K1 + K2]");
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(conv1x1_dual_supported(K1, K2, Cout, M), "conv1x1_dual: unsupported shape (K1 ", K1, ", K2 ", K2,
              ", Cout ", Cout, ")");
  auto y = torch::empty({B, Ho, Wo, Cout}, x1.options());
  conv1x1_dual_launch(hp(x1), hp(x2), hp(w), bias.data_ptr<float>(), reinterpret_cast<half_t*>(y.data_ptr()),
                      zero_buffer(dev).data_ptr(), (int)M, K1, K2, Cout, relu ? 1 : 0, H, W, Wo, Ho * Wo, (int)stride,
                      cur_stream());
  check_launch("conv1x1_dual");
  return y;
}

bool conv1x1_dual_ok(int64_t K1, int64_t K2, int64_t Cout, int64_t M) {
  return conv1x1_dual_supported((int)K1, (int)K2, (int)Cout, (long)M);
}

// Bottleneck tail + the NEXT block's reduce 1x1 in one pass (fp16, layer1 of
// ResNet50): y = relu(x1 . W^T + b + res) -- or, with x2, the dual form
// relu([x1 | x2] . W^T + b) -- and z = relu(y . w2^T + b2) from the output tile
// on chip.  Returns [y, z].
std::vector<torch::Tensor> conv1x1_fused_next(torch::Tensor x1, c10::optional<torch::Tensor> x2, torch::Tensor w,
                                              torch::Tensor bias, c10::optional<torch::Tensor> res, torch::Tensor w2,
                                              torch::Tensor b2, int64_t stride, bool relu) {
  const auto dev = x1.device();
  check_operand(x1, "x1", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, -1, dev);
  check_operand(w2, "w2", torch::kHalf, 2, dev);
  check_operand(b2, "b2", torch::kFloat, -1, dev);
  const int B = x1.size(0), Ho = x1.size(1), Wo = x1.size(2), K1 = x1.size(3);
  const int N = w.size(0), N2 = w2.size(0);
  const half_t* x2p = nullptr;
  int H = Ho, W = Wo, K2 = 0;
  if (x2.has_value() && x2->defined()) {
    auto& t = *x2;
    check_operand(t, "x2", torch::kHalf, 4, dev);
    TORCH_CHECK(t.size(0) == B, "x2 must be [B, H, W, K2]");
    H = t.size(1); W = t.size(2); K2 = t.size(3);
    TORCH_CHECK((H - 1) / stride + 1 == Ho && (W - 1) / stride + 1 == Wo, "x2 must be at `stride` of x1's resolution");
    x2p = hp(t);
  }
  TORCH_CHECK(bias.dim() >= 1 && b2.dim() >= 1 && w.size(1) == K1 + K2 && bias.size(0) == N && w2.size(1) == N &&
                  b2.size(0) == N2, "weight shapes");
  const half_t* rp = static_cast<const half_t*>(optional_res(res, dev, torch::kHalf, {B, Ho, Wo, N}));
  TORCH_CHECK(rp == nullptr || x2p == nullptr, "the dual form carries its residual as the second GEMM input");
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(conv1x1_fused_next_supported(K1, K2, N, N2, M), "conv1x1_fused_next: unsupported shape");
  auto y = torch::empty({B, Ho, Wo, N}, x1.options());
  auto z = torch::empty({B, Ho, Wo, N2}, x1.options());
  conv1x1_fused_next_launch(hp(x1), x2p, hp(w), bias.data_ptr<float>(), rp, reinterpret_cast<half_t*>(y.data_ptr()),
                            hp(w2), b2.data_ptr<float>(), reinterpret_cast<half_t*>(z.data_ptr()),
                            zero_buffer(dev).data_ptr(), (int)M, K1, K2, N, N2, relu ? 1 : 0, H, W, Wo, Ho * Wo,
                            (int)stride, cur_stream());
  check_launch("conv1x1_fused_next");
  return {y, z};
}

bool conv1x1_fused_next_ok(int64_t K1, int64_t K2, int64_t N, int64_t N2, int64_t M) {
  return conv1x1_fused_next_supported((int)K1, (int)K2, (int)N, (int)N2, (long)M);
}

// fp16 band-staged 3x3/s1/p1 conv with a persistent-grid cap (tests)
torch::Tensor conv3x3_band_f16(torch::Tensor x, torch::Tensor w, torch::Tensor bias, c10::optional<torch::Tensor> res,
                               bool relu, int64_t max_grid) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, -1, dev);
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), Cout = w.size(0);
  TORCH_CHECK(w.size(1) == 9 * C && bias.numel() == Cout, "fp16 weight must be [Cout, 9*C]");
  TORCH_CHECK(conv3x3_band_supported(H, W, C, Cout), "band conv: unsupported shape");
  auto y = torch::empty({B, H, W, Cout}, x.options());
  const half_t* rp = static_cast<const half_t*>(optional_res(res, dev, torch::kHalf, {B, H, W, Cout}));
  if (B == 0) return y;
  TORCH_CHECK(conv3x3_band_launch(hp(x), C, hp(w), bias.data_ptr<float>(), rp, Cout, y.data_ptr(), Cout, false, B, H, W,
                                  C, Cout, relu ? 1 : 0, 1.0f, nullptr, (int)max_grid, 0, cur_stream(), true),
              "band conv: tensor too large for 32-bit buffer offsets");
  check_launch("conv3x3_band (fp16)");
  return y;
}

// y = act(x @ w.T + bias) with K split over `splits` partial GEMMs (the conv
// kernel as a 1x1 conv on a K-slice of each row: ldx = K, all slices in ONE
// launch, grid = tiles x splits: one launch per slice kept each slice at the
// unsplit block count and never paid, r1 A/B) into fp32 partials, then one combine
// kernel.  For FC layers with few output tiles and a long K (AlexNet fc6-fc8 at
// batch 500: 64-256 tiles, K = 4096-9216) one tile per CU with 64-144 serial K
// stages cannot hide the DMA latency.
torch::Tensor linear_splitk(torch::Tensor x, torch::Tensor w, torch::Tensor bias, bool relu, bool out_f32,
                            int64_t splits, int64_t tile) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 2, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && bias.size(0) == N, "shape mismatch");
  TORCH_CHECK(N % 4 == 0, "N must be a multiple of 4");
  TORCH_CHECK(splits >= 1 && splits <= 16 && K % (64 * splits) == 0, "K must split into multiples of 64");
  TORCH_CHECK(M * N < (1L << 31) && M * K < (1L << 31), "too large for int32 indexing");
  auto part = torch::empty({splits, M, N}, x.options().dtype(torch::kFloat));
  auto y = torch::empty({M, N}, x.options().dtype(out_f32 ? torch::kFloat : torch::kHalf));
  if (M == 0) return y;
  const int t = tile >= 10 ? (int)tile : conv_glds_pick((int)M, (int)N);
  ConvArgs a{};
  a.x = hp(x);
  a.w = hp(w);
  fill_linear_splitk(a, M, K, N, splits, zero_f32(dev, N), part);
  TORCH_CHECK(conv_glds_launch(a, true, t, cur_stream()), "unknown conv tile id ", t);
  check_launch("linear_splitk");
  splitk_reduce_launch(part.data_ptr<float>(), (int)splits, (long)(M * N), (int)N, bias.data_ptr<float>(),
                       relu ? 1 : 0, y.data_ptr(), out_f32, cur_stream());
  check_launch("splitk_reduce");
  return y;
}
