// split-fp16 (fp32-accurate) convs and FC, the split <-> fp32 conversions, the split max pool.
#include "binding_util.h"

using namespace idunno;

static const half_t* hp(const torch::Tensor& t) { return reinterpret_cast<const half_t*>(t.data_ptr()); }

// split (fp32-accurate) form of conv1x1_dual: x1 [B, Ho, Wo, 2 K1], x2 [B, H, W, 2 K2]
// split layouts, w [Cout, 2 (K1 + K2)] = pack_split_weight([W3 | Wds]) with one
// accumulator scale; split output [B, Ho, Wo, 2 Cout] (range-guarded)
torch::Tensor conv1x1_dual_split(torch::Tensor x1, torch::Tensor x2, torch::Tensor w, torch::Tensor bias,
                                 double acc_scale, int64_t stride, bool relu) {
  const auto dev = x1.device();
  check_operand(x1, "x1", torch::kHalf, 4, dev);
  check_operand(x2, "x2", torch::kHalf, 4, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int B = x1.size(0), Ho = x1.size(1), Wo = x1.size(2), K1 = x1.size(3) / 2;
  const int H = x2.size(1), W = x2.size(2), K2 = x2.size(3) / 2;
  const int Cout = w.size(0);
  TORCH_CHECK(x1.size(3) % 64 == 0 && x2.size(3) % 64 == 0, "split inputs need 2C halfs with C % 32 == 0");
  check_strided_input(x2, B, Ho, Wo, stride);
  TORCH_CHECK(w.size(1) == 2 * (K1 + K2) && bias.size(0) == Cout, "split weight must be [Cout, 2 (K1 + K2)]");
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(conv1x1_dual_split_supported(K1, K2, Cout, M), "conv1x1_dual_split: unsupported shape (K1 ", K1,
              ", K2 ", K2, ", Cout ", Cout, ")");
  auto y = torch::empty({B, Ho, Wo, 2 * Cout}, x1.options());
  conv1x1_dual_split_launch(hp(x1), hp(x2), hp(w), bias.data_ptr<float>(), reinterpret_cast<half_t*>(y.data_ptr()),
                            zero_buffer(dev).data_ptr(), (int)M, K1, K2, Cout, relu ? 1 : 0, (float)acc_scale,
                            split_guard_for(dev), H, W, Wo, Ho * Wo, (int)stride, cur_stream());
  check_launch("conv1x1_dual_split");
  return y;
}

bool conv1x1_dual_split_ok(int64_t K1, int64_t K2, int64_t Cout, int64_t M) {
  return conv1x1_dual_split_supported((int)K1, (int)K2, (int)Cout, (long)M);
}

// split fp16 (fp32-accurate) conv: y = act(acc_scale * conv(x, w) + bias (+ res)).
//   x   : [B, H, W, 2C] half, split layout ([hi x32][lo x32] per 32 channels), C % 32 == 0;
//         an NHWC view (a channel slice of a dual conv's output) is read in place
//   w   : [Cout, KH*KW*2C] half, same layout per tap, pre-scaled by 1/acc_scale
//   res : optional [B, Ho, Wo, 2Cout] half (split, view allowed);  y: split half, or fp32 [B, Ho, Wo, Cout]
static torch::Tensor conv2d_split_impl(torch::Tensor x, torch::Tensor w, torch::Tensor bias,
                                       c10::optional<torch::Tensor> res, int64_t KH, int64_t KW, int64_t stride,
                                       int64_t pad, bool relu, double acc_scale, bool out_f32, int64_t tile,
                                       c10::optional<torch::Tensor> out, int64_t nsplit, bool center_only,
                                       double acc_scale2, int64_t ksplit, int64_t route) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 4, dev, false);
  const int64_t xP = nhwc_pixel_stride(x, "x");
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  TORCH_CHECK(KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0, "bad conv geometry");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C2 = x.size(3);
  TORCH_CHECK(C2 % 64 == 0, "split input needs 2C halfs with C % 32 == 0, got ", C2);
  const int Cout = w.size(0), Kpad = w.size(1);
  TORCH_CHECK(Kpad == KH * KW * C2, "split weight must be [Cout, KH*KW*2C]");
  TORCH_CHECK(bias.size(0) == Cout, "bias/Cout mismatch");
  TORCH_CHECK(Cout % 32 == 0, "split conv needs Cout % 32 == 0");
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty output");
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(M < (1L << 31) && (long)B * H * W * xP < (1L << 31) && M * 2 * Cout < (1L << 31),
              "tensor too large for int32 indexing");
  const int64_t ych = out_f32 ? Cout : 2 * Cout;
  auto y = optional_out(out, dev, out_f32 ? torch::kFloat : torch::kHalf, {B, Ho, Wo, ych});
  int64_t rP = 2 * Cout;
  const half_t* rp = static_cast<const half_t*>(optional_res(res, dev, torch::kHalf, {B, Ho, Wo, 2 * Cout}, &rP));
  ConvArgs a{};
  a.x = hp(x);
  a.w = hp(w);
  a.bias = bias.data_ptr<float>();
  a.res = rp;
  a.y = y.data_ptr();
  fill_conv_geometry(a, B, H, W, C2, Ho, Wo, Cout, (int)ych, KH, KW, stride, pad, M, Kpad, relu);
  a.acc_scale = (float)acc_scale;
  a.ovf = out_f32 ? nullptr : split_guard_for(dev);
  // strided views (a dual conv's halves): conv_glds reads them in place
  const bool strided = xP != C2 || rP != 2 * Cout;
  a.ldx = xP != C2 ? (int)xP : 0;
  a.ldr = rP != 2 * Cout ? (int)rP : 0;
  TORCH_CHECK(nsplit >= 0 && nsplit < Cout && nsplit % 32 == 0, "dual conv split must be a multiple of 32 below Cout");
  a.nsplit_n = (int)nsplit;
  a.center_only = center_only ? 1 : 0;
  a.acc_scale2 = (float)acc_scale2;
  TORCH_CHECK(!center_only || (nsplit > 0 && KH % 2 == 1 && KW % 2 == 1 && pad == KH / 2 && pad == KW / 2),
              "centre-only dual conv needs an odd, 'same'-padded kernel");
  if (M == 0) return y;
  a.zero = zero_buffer(dev).data_ptr();
  const bool c64_ok = KH == 3 && KW == 3 && stride == 1 && pad == 1 && !out_f32 && !strided && nsplit == 0 &&
                      conv3x3_split_c64_supported(H, W, C2 / 2, Cout);
  // row-streaming register-weight kernel for split 3x3/s1 64->64 (ResNet layer1)
  if (tile == 50 || (tile < 0 && c64_ok && !(route & kRouteNoC64))) {
    TORCH_CHECK(c64_ok, "tile 50 (row-streaming split 3x3 64->64 conv) does not support this shape");
    TORCH_CHECK(conv3x3_split_c64_launch(a.x, a.w, a.bias, a.res, reinterpret_cast<half_t*>(a.y), a.zero, B, H, W,
                                         a.relu, a.acc_scale, a.ovf, cur_stream(), (route & kRouteC64TwoPerCU) ? 2 : 0),
                "row-streaming split conv: tensor too large for 32-bit offsets");
    check_launch("conv3x3_split_c64");
    return y;
  }
  // band-staged 3x3 kernel (conv3x3_band.hip, tile 70): ResNet layers 2 and 4 at batches
  // that give every CU a tile (conv3x3_band_default; otherwise the im2col tiles + split-K)
  const bool band_ok = KH == 3 && KW == 3 && stride == 1 && pad == 1 && nsplit == 0 &&
                       conv3x3_band_supported(H, W, C2 / 2, Cout);
  const bool band_off = (route & kRouteNoBand) || (W == 28 && (route & kRouteNoBandW28));
  const bool band_on = conv3x3_band_default(B, W, Cout) ||
                       (W == 7 && (route & kRouteBandW7) && conv3x3_band_tiles(B, W, Cout) >= device_cu_count());
  if (tile == 70 || (tile < 0 && band_ok && !band_off && band_on)) {
    TORCH_CHECK(band_ok, "tile 70 (band-staged split 3x3 conv) does not support this shape");
    TORCH_CHECK(conv3x3_band_launch(a.x, (int)xP, a.w, a.bias, rp, (int)rP, a.y, (int)ych, out_f32, B, H, W, C2 / 2,
                                    Cout, a.relu, a.acc_scale, a.ovf, 0, 0, cur_stream()),
                "band conv: tensor too large for 32-bit buffer offsets");
    check_launch("conv3x3_band");
    return y;
  }
  const bool c1s_ok = KH == 1 && KW == 1 && (stride == 1 || stride == 2) && pad == 0 && !out_f32 && !strided &&
                      nsplit == 0 && conv1x1_stream_split_supported(C2 / 2, Cout, M);
  const bool legacy_small = (route & kRouteLegacySmallM) != 0;
  if (tile == 80 || (tile < 0 && c1s_ok && !(route & kRouteNoStream1x1) && conv1x1_stream_split_default(C2 / 2, stride) &&
                     (legacy_small || !conv1x1_small_m(M)))) {
    TORCH_CHECK(c1s_ok, "tile 80 (streaming split 1x1 conv) does not support this shape");
    conv1x1_stream_split_launch(a.x, a.w, a.bias, a.res, reinterpret_cast<half_t*>(a.y), a.zero, a.M, C2 / 2, Cout,
                                a.relu, a.acc_scale, a.ovf, H, W, Wo, Ho * Wo, stride, cur_stream());
    check_launch("conv1x1_stream_split");
    return y;
  }
  // a small-M 1x1 (the downsample at a few dozen images per GPU) on the 128 x 64 tile
  // (a forced ksplit > 1 keeps the split-K tile: tests drive that path at small M)
  const bool small_1x1 = KH == 1 && KW == 1 && !legacy_small && conv1x1_small_m(M) && Cout % 128 == 0 && ksplit <= 1;
  const int t = tile >= 0 ? (int)tile : (small_1x1 ? 38 : conv_glds_split_pick(a.M, Cout));
  const int nk_total = (int)(KH * KW) * (C2 / 64);
  // split-K: auto only for the auto-picked tile (a forced tile runs its own epilogue)
  const int ks = nsplit == 0 ? conv_split_ksplit(a.M, Cout, t, nk_total, tile >= 0 && ksplit < 0 ? 1 : (int)ksplit,
                                                 legacy_small)
                             : 1;
  TORCH_CHECK(ksplit <= 1 || ks == ksplit, "split-K: ", ksplit, " slices do not divide the K loop of tile ", t);
  if (ks > 1) {
    // small M: K slices into fp32 partials in one launch, then one combine
    // (bias, residual, ReLU, split + range guard) -- conv_glds.hip conv_split_ksplit
    TORCH_CHECK((long)ks * M * Cout < (1L << 31), "split-K partials too large for int32 indexing");
    auto part = torch::empty({ks, M, (int64_t)Cout}, x.options().dtype(torch::kFloat));
    auto zb = zero_f32(dev, Cout);
    ConvArgs b = a;
    b.bias = zb.data_ptr<float>();
    b.res = nullptr;
    b.ldr = 0;
    b.y = part.data_ptr<float>();
    b.ldy = Cout;
    b.relu = 0;
    b.ovf = nullptr;
    b.ksplit = ks;
    b.kslice = 0;
    b.ysplit = (long)M * Cout;
    b.kstage = nk_total / ks;
    TORCH_CHECK(conv_glds_split_launch(b, true, t, cur_stream()), "unknown split conv tile id ", t);
    check_launch("conv_glds_split (split-K)");
    splitk_reduce_res_launch(part.data_ptr<float>(), ks, (long)M * Cout, Cout, a.bias, rp, (int)rP, a.relu, a.y,
                             (int)ych, out_f32 ? 1 : 0, a.ovf, cur_stream());
    check_launch("splitk_reduce_res");
    return y;
  }
  TORCH_CHECK(conv_glds_split_launch(a, out_f32, t, cur_stream()), "unknown split conv tile id ", t);
  check_launch("conv_glds_split");
  return y;
}

// Band-staged split 3x3/s1/p1 conv with an explicit persistent-grid cap (tests:
// max_grid < tiles makes every workgroup run several tiles through one DMA ring).
torch::Tensor conv3x3_band_split(torch::Tensor x, torch::Tensor w, torch::Tensor bias, c10::optional<torch::Tensor> res,
                                 bool relu, double acc_scale, bool out_f32, int64_t max_grid, int64_t flags) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 4, dev, false);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, -1, dev);
  const int64_t xP = nhwc_pixel_stride(x, "x");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C2 = x.size(3), Cout = w.size(0);
  TORCH_CHECK(w.size(1) == 9 * C2 && bias.numel() == Cout, "split weight must be [Cout, 9*2C]");
  TORCH_CHECK(conv3x3_band_supported(H, W, C2 / 2, Cout), "band conv: unsupported shape");
  const int64_t ych = out_f32 ? Cout : 2 * Cout;
  auto y = torch::empty({B, H, W, ych}, x.options().dtype(out_f32 ? torch::kFloat : torch::kHalf));
  int64_t rP = 2 * Cout;
  const half_t* rp = static_cast<const half_t*>(optional_res(res, dev, torch::kHalf, {B, H, W, 2 * Cout}, &rP));
  if (B == 0) return y;
  TORCH_CHECK(conv3x3_band_launch(hp(x), (int)xP, hp(w), bias.data_ptr<float>(), rp, (int)rP, y.data_ptr(), (int)ych,
                                  out_f32, B, H, W, C2 / 2, Cout, relu ? 1 : 0, (float)acc_scale,
                                  out_f32 ? nullptr : split_guard_for(dev), (int)max_grid, (int)flags, cur_stream()),
              "band conv: tensor too large for 32-bit buffer offsets");
  check_launch("conv3x3_band");
  return y;
}

torch::Tensor conv2d_split(torch::Tensor x, torch::Tensor w, torch::Tensor bias, c10::optional<torch::Tensor> res,
                           int64_t KH, int64_t KW, int64_t stride, int64_t pad, bool relu, double acc_scale,
                           bool out_f32, int64_t tile, c10::optional<torch::Tensor> out, int64_t ksplit,
                           int64_t route) {
  return conv2d_split_impl(x, w, bias, res, KH, KW, stride, pad, relu, acc_scale, out_f32, tile, out, 0, false, 1.0,
                           ksplit, route);
}

// Two split convs of one input in ONE launch (the ResNet stride-2
// block's 1x1/2 downsample is the centre tap of its 3x3/2 conv): w / bias are
// [Cout1 + Cout2, ...] with the second conv's weights in the centre-tap K block
// (zeros elsewhere, never read); output channels [0, nsplit) = conv 1 (ReLU if
// relu, scale acc_scale), [nsplit, Cout) = conv 2 (no ReLU, scale acc_scale2,
// K loop over the centre tap only when center_only).  y = [B, Ho, Wo, 2*Cout]
// split; its channel halves are read in place by the next convs (pixel stride).
torch::Tensor conv2d_split_dual(torch::Tensor x, torch::Tensor w, torch::Tensor bias, int64_t KH, int64_t KW,
                                int64_t stride, int64_t pad, bool relu, double acc_scale, double acc_scale2,
                                int64_t nsplit, bool center_only, int64_t tile) {
  TORCH_CHECK(nsplit > 0, "dual conv needs nsplit > 0");
  return conv2d_split_impl(x, w, bias, c10::nullopt, KH, KW, stride, pad, relu, acc_scale, false, tile,
                           c10::nullopt, nsplit, center_only, acc_scale2, 1, 0);
}

// A residual block's second 3x3/s1/p1 conv with its 1x1 pad-0 downsample as a K
// tail (conv_glds.hip TAIL): out = act(acc_scale * (conv3x3(y, W2) + conv1x1/stride2(x2, Wd)) + bias)
// as ONE GEMM over K = [9 taps of y | channels of x2 at the strided pixel].
//   y  : [B, Ho, Wo, 2C] split     x2 : [B, H2, W2, 2Cx] split, Ho == (H2 - 1) / stride2 + 1 (same for W)
//   w  : [Cout, 9*2C + 2Cx] split, one exponent (models/packed.py pack_split_weight of both parts)
// Not the fuse_down / conv2d_split_dual path above, which fuses the downsample into
// the block's FIRST conv and still writes and re-reads the identity.
torch::Tensor conv2d_split_tail(torch::Tensor y, torch::Tensor x2, torch::Tensor w, torch::Tensor bias,
                                double acc_scale, int64_t stride2, bool relu, int64_t tile) {
  const auto dev = y.device();
  check_operand(y, "y", torch::kHalf, 4, dev, false);
  check_operand(x2, "x2", torch::kHalf, 4, dev, false);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t yP = nhwc_pixel_stride(y, "y"), xP = nhwc_pixel_stride(x2, "x2");
  const int B = y.size(0), Ho = y.size(1), Wo = y.size(2), C2 = y.size(3);
  const int H2 = x2.size(1), W2 = x2.size(2), Cx2 = x2.size(3), Cout = w.size(0);
  TORCH_CHECK(C2 % 64 == 0 && Cx2 % 64 == 0 && Cx2 > 0, "split operands need 2C halfs with C % 32 == 0");
  TORCH_CHECK(w.size(1) == 9 * (int64_t)C2 + Cx2, "tail weight must be [Cout, 9*2C + 2Cx]");
  TORCH_CHECK(bias.size(0) == Cout && Cout % 32 == 0, "bias/Cout mismatch, or Cout % 32 != 0");
  TORCH_CHECK(stride2 >= 1 && x2.size(0) == B && Ho == (H2 - 1) / stride2 + 1 && Wo == (W2 - 1) / stride2 + 1,
              "x2 geometry does not give y's [B, Ho, Wo] at this stride");
  const long M = (long)B * Ho * Wo;
  TORCH_CHECK(M * yP < (1L << 31) && (long)B * H2 * W2 * xP < (1L << 31) && M * 2 * Cout < (1L << 31),
              "tensor too large for int32 indexing");
  auto out = torch::empty({B, Ho, Wo, 2 * (int64_t)Cout}, y.options());
  if (M == 0) return out;
  ConvArgs a{};
  a.x = hp(y);
  a.w = hp(w);
  a.bias = bias.data_ptr<float>();
  a.y = out.data_ptr();
  fill_conv_geometry(a, B, Ho, Wo, C2, Ho, Wo, Cout, 2 * Cout, 3, 3, 1, 1, M, (int)w.size(1), relu);
  a.acc_scale = (float)acc_scale;
  a.ovf = split_guard_for(dev);
  a.ldx = yP != C2 ? (int)yP : 0;
  a.zero = zero_buffer(dev).data_ptr();
  a.x2 = hp(x2);
  a.H2 = H2; a.W2 = W2; a.ldx2 = (int)xP; a.stride2 = (int)stride2;
  a.cblk2 = Cx2 / 64;
  const int t = tile >= 0 ? (int)tile : conv_glds_split_tail_pick(a.M, Cout);
  TORCH_CHECK(conv_glds_split_tail_launch(a, t, cur_stream()), "conv2d_split_tail: tile ", t,
              " has no K-tail form (36 / 42)");
  check_launch("conv_glds_split (K tail)");
  return out;
}

// whether models/packed.py fuses a block's downsample into its second 3x3 conv by default
// (the modes of conv_split_tail_default: 1 the rule, 2 every supported shape, 3 the rule minus the band
// kernel's shapes)
bool conv2d_split_tail_ok(int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Cx, int64_t Cout, int64_t mode) {
  return conv_split_tail_default((int)B, (int)Ho, (int)Wo, (int)C, (int)Cx, (int)Cout, (int)mode);
}

// fp32-accurate FC on split fp16: y = act(acc_scale * x @ w.T + bias)
//   x [M, 2K] split, w [N, 2K] split (pack_split_weight of [N, K, 1, 1]); K % 32 == 0.
// K is cut into `splits` slices in ONE conv_glds launch (fp32 partials) + the
// combine, which writes fp32 [M, N] or split [M, 2N] (N % 32 == 0).
torch::Tensor linear_split(torch::Tensor x, torch::Tensor w, torch::Tensor bias, double acc_scale, bool relu,
                           bool out_f32, int64_t splits, int64_t tile) {
  const auto dev = x.device();
  check_operand(x, "x", torch::kHalf, 2, dev);
  check_operand(w, "w", torch::kHalf, 2, dev);
  check_operand(bias, "bias", torch::kFloat, 1, dev);
  const int64_t M = x.size(0), K2 = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K2 && bias.size(0) == N, "shape mismatch");
  TORCH_CHECK(out_f32 ? N % 4 == 0 : N % 32 == 0, "N must be a multiple of 4 (fp32 out) / 32 (split out)");
  TORCH_CHECK(splits >= 1 && splits <= 16 && K2 % (64 * splits) == 0, "K must split into multiples of 32");
  TORCH_CHECK(splits * M * N < (1L << 31) && M * K2 < (1L << 31), "too large for int32 indexing");
  auto part = torch::empty({splits, M, N}, x.options().dtype(torch::kFloat));
  auto y = out_f32 ? torch::empty({M, N}, x.options().dtype(torch::kFloat))
                   : torch::empty({M, 2 * N}, x.options().dtype(torch::kHalf));
  if (M == 0) return y;
  ConvArgs a{};
  a.x = hp(x);
  a.w = hp(w);
  fill_linear_splitk(a, M, K2, N, splits, zero_f32(dev, N), part);
  a.acc_scale = (float)acc_scale;
  const int t = tile >= 0 ? (int)tile : conv_glds_split_pick((int)M, (int)N);
  TORCH_CHECK(conv_glds_split_launch(a, true, t, cur_stream()), "unknown split conv tile id ", t);
  check_launch("linear_split");
  if (out_f32)
    splitk_reduce_launch(part.data_ptr<float>(), (int)splits, (long)(M * N), (int)N, bias.data_ptr<float>(),
                         relu ? 1 : 0, y.data_ptr(), true, cur_stream());
  else
    splitk_reduce_split_launch(part.data_ptr<float>(), (int)splits, (long)(M * N), (int)N, bias.data_ptr<float>(),
                               relu ? 1 : 0, reinterpret_cast<half_t*>(y.data_ptr()), split_guard_for(dev),
                               cur_stream());
  check_launch("splitk_reduce");
  return y;
}

// fp32 NHWC [.., C] <-> split [.., 2C] (C % 32 == 0)
torch::Tensor split_from_f32(torch::Tensor x) {
  check_operand(x, "x", torch::kFloat, -1, x.device());
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) % 32 == 0, "last dim must be a multiple of 32");
  const int C = x.size(-1);
  auto sz = x.sizes().vec();
  sz.back() = 2 * C;
  auto y = torch::empty(sz, x.options().dtype(torch::kHalf));
  const long npix = C ? x.numel() / C : 0;
  if (npix == 0) return y;
  split_from_f32_launch(x.data_ptr<float>(), reinterpret_cast<half_t*>(y.data_ptr()), npix, C,
                        split_guard_for(x.device()), cur_stream());
  check_launch("split_from_f32");
  return y;
}

torch::Tensor f32_from_split(torch::Tensor x) {
  check_operand(x, "x", torch::kHalf, -1, x.device());
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) % 64 == 0, "last dim must be 2C with C % 32 == 0");
  const int C = x.size(-1) / 2;
  auto sz = x.sizes().vec();
  sz.back() = C;
  auto y = torch::empty(sz, x.options().dtype(torch::kFloat));
  const long npix = x.numel() / (2 * C);
  if (npix == 0) return y;
  f32_from_split_launch(hp(x), y.data_ptr<float>(), npix, C, cur_stream());
  check_launch("f32_from_split");
  return y;
}

// NHWC max pool into the split layout; x fp32 [B,H,W,C] or split half [B,H,W,2C]
torch::Tensor maxpool2d_split(torch::Tensor x, int64_t k, int64_t s, int64_t pad, c10::optional<torch::Tensor> out) {
  const bool in_split = x.scalar_type() == torch::kHalf;
  TORCH_CHECK(in_split || x.scalar_type() == torch::kFloat, "x must be fp32 or split half");
  check_operand(x, "x", x.scalar_type(), 4, x.device());
  TORCH_CHECK(k >= 1 && s >= 1 && pad >= 0 && pad < k, "bad pool geometry");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = in_split ? x.size(3) / 2 : x.size(3);
  TORCH_CHECK(C % 32 == 0 && (!in_split || x.size(3) == 2 * C), "channels must be a multiple of 32");
  const int Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty output");
  auto y = optional_out(out, x.device(), torch::kHalf, {B, Ho, Wo, 2 * C});
  if ((long)B * Ho * Wo == 0) return y;
  maxpool_split_launch(x.data_ptr(), in_split, reinterpret_cast<half_t*>(y.data_ptr()), B, H, W, C, Ho, Wo, k, s, pad,
                       split_guard_for(x.device()), cur_stream());
  check_launch("maxpool_split");
  return y;
}
