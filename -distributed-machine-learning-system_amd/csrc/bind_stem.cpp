// uint8 image front ends: the fused stems, preprocess*, resize_crop*.
//
// Device-side window (every entry point with `start`): with `start` (int64 GPU
// scalar) and batch > 0, `img` is a whole image shard [N,H,W,3] and images
// [*start, *start + batch) are used; the kernel clamps *start into [0, N - batch]
// so a bad descriptor can never read outside the shard.  A window may be
// processed in parts: `window` (>= batch, default batch) is the clamping window,
// `sub` this launch's first image inside it (sub + batch <= window).
// `start_offset` is subtracted from *start on the device: the window start may be
// a GLOBAL image index (e.g. straight from the broadcast query descriptor) and the
// offset the shard's first global index.
#include "binding_util.h"

using namespace idunno;

// The image and window part every uint8 front end shares: img [N, H, W, 3] uint8.
struct StemImage {
  int B, H, W;
  const long long* sp;      // device window start, or null
  long long max_start;
};
static StemImage stem_image(const torch::Tensor& img, const c10::optional<torch::Tensor>& start, int64_t batch,
                            int64_t window, int64_t sub) {
  check_operand(img, "img", torch::kUInt8, 4, img.device());
  TORCH_CHECK(img.size(3) == 3, "img must be [B, H, W, 3] uint8");
  StemImage s;
  s.H = img.size(1);
  s.W = img.size(2);
  s.sp = window_args(img, start, batch, window, sub, s.B, s.max_start);
  return s;
}
// ... of a conv stem with a K x K kernel
static StemImage stem_image(const torch::Tensor& img, const c10::optional<torch::Tensor>& start, int64_t batch,
                            int64_t window, int64_t sub, int K) {
  const StemImage s = stem_image(img, start, batch, window, sub);
  TORCH_CHECK(s.H >= K && s.W >= K, "image too small");
  TORCH_CHECK((long)s.B * s.H * s.W * 3 < (1L << 31), "batch too large");
  return s;
}

// uint8 [B,H,W,3] -> maxpool3x3/2(relu(conv7x7/2(normalise(img)) + bias)) : fp16 [B,Hp,Wp,64]
torch::Tensor stem_fused(torch::Tensor img, torch::Tensor w, torch::Tensor bias, c10::optional<torch::Tensor> start,
                         int64_t batch, int64_t start_offset, int64_t window, int64_t sub) {
  const StemImage s = stem_image(img, start, batch, window, sub, 7);
  check_operand(w, "w", torch::kHalf, 2, img.device());
  check_operand(bias, "bias", torch::kFloat, -1, img.device());
  TORCH_CHECK(w.size(0) == 64 && w.size(1) == 7 * 32, "stem weight must be [64, 7*32] (small-C packing)");
  TORCH_CHECK(bias.numel() == 64, "bias must have 64 entries");
  const int Hc = (s.H + 6 - 7) / 2 + 1, Wc = (s.W + 6 - 7) / 2 + 1;
  const int Hp = (Hc + 2 - 3) / 2 + 1, Wp = (Wc + 2 - 3) / 2 + 1;
  auto y = torch::empty({s.B, Hp, Wp, 64}, img.options().dtype(torch::kHalf));
  if (s.B)
    stem_fused_launch(img.data_ptr<uint8_t>(), reinterpret_cast<const half_t*>(w.data_ptr()), bias.data_ptr<float>(),
                      reinterpret_cast<half_t*>(y.data_ptr()), s.B, s.H, s.W, s.sp, start_offset, s.max_start,
                      s.sp ? sub : 0, cur_stream());
  check_launch("stem_fused");
  return y;
}

// The four exact-u8 stems (uint8 image -> conv K x K -> bias, ReLU -> max pool 3x3/2) differ in
// these constants only; (w, bias, psum, acc_scale) = models/packed.py pack_stem_split /
// pack_alex_stem_split: w [2, 64, wk*32] hi/lo, psum [ps, ps, 64] border prefix sums.
struct ExactStem {
  const char* name;
  int K, stride, pad, pool_pad;   // conv kernel / stride / pad; pad of the 3x3/2 max pool
  int wk, ps;                     // K steps of the weight, prefix-sum side
  int cout;                       // output halfs per pixel: 128 split, 64 fp16
  int bound;                      // int32 output bound: B*Hp*Wp*bound < 2^31
  bool (*launch)(const uint8_t* img, const half_t* w, const float* bias, const float* psum, float acc_scale,
                 half_t* y, const StemImage& s, long long start_off, long long sub, int* guard, int form,
                 hipStream_t st);
  bool guarded;                   // split output: range-guarded
};

static torch::Tensor exact_stem(const ExactStem& k, const torch::Tensor& img, const torch::Tensor& w,
                                const torch::Tensor& bias, const torch::Tensor& psum, double acc_scale,
                                const c10::optional<torch::Tensor>& start, int64_t batch, int64_t start_offset,
                                int64_t window, int64_t sub, int64_t form) {
  const StemImage s = stem_image(img, start, batch, window, sub, k.K);
  check_operand(w, "w", torch::kHalf, 3, img.device());
  check_operand(bias, "bias", torch::kFloat, -1, img.device());
  check_operand(psum, "psum", torch::kFloat, -1, img.device());
  TORCH_CHECK(w.size(0) == 2 && w.size(1) == 64 && w.size(2) == k.wk * 32, k.name, ": weight must be [2, 64, ", k.wk,
              "*32]");
  TORCH_CHECK(bias.numel() == 64, "bias must have 64 entries");
  TORCH_CHECK(psum.numel() == k.ps * k.ps * 64, "psum must be [", k.ps, ", ", k.ps, ", 64]");
  TORCH_CHECK(form >= -1 && form <= 1, k.name, ": form must be -1 (default), 0 (one-half workgroups) or 1 (phased)");
  const int Hc = (s.H + 2 * k.pad - k.K) / k.stride + 1, Wc = (s.W + 2 * k.pad - k.K) / k.stride + 1;
  TORCH_CHECK(Hc + 2 * k.pool_pad >= 3 && Wc + 2 * k.pool_pad >= 3, "image too small for the pool");
  const int Hp = (Hc + 2 * k.pool_pad - 3) / 2 + 1, Wp = (Wc + 2 * k.pool_pad - 3) / 2 + 1;
  TORCH_CHECK((long)s.B * Hp * Wp * k.bound < (1L << 31), "batch too large");
  auto y = torch::empty({s.B, Hp, Wp, k.cout}, img.options().dtype(torch::kHalf));
  if (s.B) {
    TORCH_CHECK(k.launch(img.data_ptr<uint8_t>(), reinterpret_cast<const half_t*>(w.data_ptr()),
                         bias.data_ptr<float>(), psum.data_ptr<float>(), (float)acc_scale,
                         reinterpret_cast<half_t*>(y.data_ptr()), s, start_offset, s.sp ? sub : 0,
                         k.guarded ? split_guard_for(img.device()) : nullptr, (int)form, cur_stream()),
                k.name, ": bad geometry");
    check_launch(k.name);
  }
  return y;
}

#define STEM_LAUNCH(call)                                                                                         \
  [](const uint8_t* img, const half_t* w, const float* bias, const float* psum, float acc_scale, half_t* y,       \
     const StemImage& s, long long off, long long sub, int* guard, int form, hipStream_t st) -> bool {            \
    (void)guard; (void)form;                                                                                       \
    call;                                                                                                          \
    return true;                                                                                                   \
  }
#define STEM_ARGS img, w, bias, psum, acc_scale, y, s.B, s.H, s.W, s.sp, off, s.max_start, sub

// AlexNet: conv 11x11/4 pad 2, pool without padding (alex_stem.hip); `form` picks the kernel.
// alex_stem_u8_f16 keeps the `* 128` bound it always had although it writes 64 halfs per pixel.
static const ExactStem kAlexSplit{"alex_stem_split", 11, 4, 2, 0, 17, 12, 128, 128,
                                  STEM_LAUNCH(return alex_stem_split_launch(STEM_ARGS, guard, form, st)), true};
static const ExactStem kAlexF16{"alex_stem_u8_f16", 11, 4, 2, 0, 17, 12, 64, 128,
                                STEM_LAUNCH(return alex_stem_u8_f16_launch(STEM_ARGS, form, st)), false};
// ResNet: conv 7x7/2 pad 3, pool pad 1 (stem_fused.hip)
static const ExactStem kResSplit{"stem_split", 7, 2, 3, 1, 7, 8, 128, 128,
                                 STEM_LAUNCH(stem_split_launch(STEM_ARGS, guard, st)), true};
static const ExactStem kResF16{"stem_u8_f16", 7, 2, 3, 1, 7, 8, 64, 64,
                               STEM_LAUNCH(stem_u8_f16_launch(STEM_ARGS, st)), false};

// uint8 [B,H,W,3] -> split [B,Hp,Wp,128], fp32-accurate (form: -1 default = phased, 0 one-half, 1 phased)
torch::Tensor alex_stem_split(torch::Tensor img, torch::Tensor w, torch::Tensor bias, torch::Tensor psum,
                              double acc_scale, c10::optional<torch::Tensor> start, int64_t batch,
                              int64_t start_offset, int64_t window, int64_t sub, int64_t form) {
  return exact_stem(kAlexSplit, img, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, form);
}
// fp16 programs: hi MFMA only, fp16 [B,Hp,Wp,64] (form: -1 default = 0 two one-half workgroups per CU, 1 phased)
torch::Tensor alex_stem_u8_f16(torch::Tensor img, torch::Tensor w, torch::Tensor bias, torch::Tensor psum,
                               double acc_scale, c10::optional<torch::Tensor> start, int64_t batch,
                               int64_t start_offset, int64_t window, int64_t sub, int64_t form) {
  return exact_stem(kAlexF16, img, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, form);
}
torch::Tensor stem_split(torch::Tensor img, torch::Tensor w, torch::Tensor bias, torch::Tensor psum, double acc_scale,
                         c10::optional<torch::Tensor> start, int64_t batch, int64_t start_offset, int64_t window,
                         int64_t sub) {
  return exact_stem(kResSplit, img, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, -1);
}
torch::Tensor stem_u8_f16(torch::Tensor img, torch::Tensor w, torch::Tensor bias, torch::Tensor psum, double acc_scale,
                          c10::optional<torch::Tensor> start, int64_t batch, int64_t start_offset, int64_t window,
                          int64_t sub) {
  return exact_stem(kResF16, img, w, bias, psum, acc_scale, start, batch, start_offset, window, sub, -1);
}

torch::Tensor preprocess(torch::Tensor img, c10::optional<torch::Tensor> start, int64_t batch, int64_t start_offset,
                         int64_t window, int64_t sub, bool f32) {
  const StemImage s = stem_image(img, start, batch, window, sub);
  auto out = torch::empty({s.B, s.H, s.W, 4}, img.options().dtype(f32 ? torch::kFloat : torch::kHalf));
  const long npix = (long)s.B * s.H * s.W;
  if (!npix) return out;
  if (f32) {
    preprocess_f32_launch(img.data_ptr<uint8_t>(), out.data_ptr<float>(), npix, s.sp, start_offset, s.max_start,
                          s.sp ? sub : 0, (long)s.H * s.W, cur_stream());
    check_launch("preprocess_f32");
    return out;
  }
  preprocess_launch(img.data_ptr<uint8_t>(), reinterpret_cast<half_t*>(out.data_ptr()), npix, s.sp, start_offset,
                    s.max_start, s.sp ? sub : 0, (long)s.H * s.W, cur_stream());
  check_launch("preprocess");
  return out;
}

// uint8 [B, H, W, 3] -> packed-row stem input [B, H, copies * nc, wp] for a KW-wide, stride-`stride`,
// pad-`pad` stem; dtype 0 fp32, 1 fp16 (conv2d_pack3), 2 split fp16 = hi copies then lo copies
// (conv2d_pack3_split).  Same window arguments as preprocess.
static torch::Tensor pack3_rows(const torch::Tensor& img, int64_t KW, int64_t stride, int64_t pad,
                                const c10::optional<torch::Tensor>& start, int64_t batch, int64_t start_offset,
                                int64_t window, int64_t sub, int dtype) {
  const StemImage s = stem_image(img, start, batch, window, sub);
  TORCH_CHECK(KW >= 5 && stride >= 1 && pad >= 0, "pack3 stem geometry: KW >= 5");
  int nc, wp, cpk;
  pack3_geometry(s.W, (int)KW, (int)stride, (int)pad, dtype ? 2 : 4, nc, wp, cpk);
  TORCH_CHECK(nc <= 4, "pack3 stem: stride needs at most 4 row copies");
  const int copies = dtype == 2 ? 2 : 1;
  TORCH_CHECK((long)s.B * s.H * copies * nc * wp < (1L << 31), "tensor too large for int32 indexing");
  auto out = torch::empty({s.B, s.H, copies * nc, wp}, img.options().dtype(dtype ? torch::kHalf : torch::kFloat));
  if (s.B == 0) return out;
  const uint8_t* ip = img.data_ptr<uint8_t>();
  half_t* oh = reinterpret_cast<half_t*>(out.data_ptr());
  const long long sb = s.sp ? sub : 0;
  if (dtype == 2) {
    preprocess_pack3_split_launch(ip, oh, s.B, s.H, s.W, (int)pad, nc, wp, s.sp, start_offset, s.max_start, sb,
                                  cur_stream());
    check_launch("preprocess_pack3_split");
  } else if (dtype == 1) {
    preprocess_pack3_f16_launch(ip, oh, s.B, s.H, s.W, (int)pad, nc, wp, s.sp, start_offset, s.max_start, sb,
                                cur_stream());
    check_launch("preprocess_pack3_f16");
  } else {
    preprocess_pack3_f32_launch(ip, out.data_ptr<float>(), s.B, s.H, s.W, (int)pad, nc, wp, s.sp, start_offset,
                                s.max_start, sb, cur_stream());
    check_launch("preprocess_pack3_f32");
  }
  return out;
}

torch::Tensor preprocess_pack3(torch::Tensor img, int64_t KW, int64_t stride, int64_t pad,
                               c10::optional<torch::Tensor> start, int64_t batch, int64_t start_offset,
                               int64_t window, int64_t sub, bool f16) {
  return pack3_rows(img, KW, stride, pad, start, batch, start_offset, window, sub, f16 ? 1 : 0);
}

torch::Tensor preprocess_pack3_split(torch::Tensor img, int64_t KW, int64_t stride, int64_t pad,
                                     c10::optional<torch::Tensor> start, int64_t batch, int64_t start_offset,
                                     int64_t window, int64_t sub) {
  return pack3_rows(img, KW, stride, pad, start, batch, start_offset, window, sub, 2);
}

// Host only: (Hr, Wr, top, left) of Resize(shorter side -> resize) + CenterCrop(crop) on an
// Hi x Wi image (tile_math.h resize_crop_geometry), the one definition resize_crop uses.
// The offsets mean something only where the crop fits (Hr >= crop and Wr >= crop).
std::tuple<int64_t, int64_t, int64_t, int64_t> resize_crop_geometry_py(int64_t Hi, int64_t Wi, int64_t resize,
                                                                       int64_t crop) {
  TORCH_CHECK(Hi >= 1 && Wi >= 1 && resize >= 1 && crop >= 1, "resize_crop_geometry: sizes must be positive");
  TORCH_CHECK(Hi < (1 << 24) && Wi < (1 << 24) && resize < (1 << 24) && crop < (1 << 24) &&
                  resize * std::max(Hi, Wi) / std::min(Hi, Wi) < (1 << 24),
              "resize_crop_geometry: image too large");
  int Hr, Wr, top, left;
  resize_crop_geometry((int)Hi, (int)Wi, (int)resize, (int)crop, Hr, Wr, top, left);
  return {Hr, Wr, top, left};
}

torch::Tensor resize_crop(torch::Tensor img, int64_t resize, int64_t crop) {
  check_operand(img, "img", torch::kUInt8, 4, img.device());
  TORCH_CHECK(img.size(3) == 3, "img must be [B, H, W, 3] uint8");
  const int B = img.size(0), Hi = img.size(1), Wi = img.size(2);
  TORCH_CHECK(B == 0 || (Hi >= 1 && Wi >= 1), "empty image");
  auto out = torch::empty({B, crop, crop, 4}, img.options().dtype(torch::kHalf));
  if (!B) return out;
  const auto [Hr, Wr, top, left] = resize_crop_geometry_py(Hi, Wi, resize, crop);
  TORCH_CHECK(Hr >= crop && Wr >= crop, "crop larger than resized image");
  resize_crop_launch(img.data_ptr<uint8_t>(), reinterpret_cast<half_t*>(out.data_ptr()), B, Hi, Wi, (int)Hr, (int)Wr,
                     crop, (int)top, (int)left, cur_stream());
  check_launch("resize_crop");
  return out;
}
