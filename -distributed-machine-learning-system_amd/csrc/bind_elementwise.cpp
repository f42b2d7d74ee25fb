// Memory-bound ops and small utilities: pools, softmax_top1 / softmax_topk, synth_images, graph_launch, tile pickers.
#include "binding_util.h"

using namespace idunno;

// fp16 or fp32 NHWC [B, H, W, C] with C % 8 (fp16) / 4 (fp32) == 0; returns whether it is fp32
static bool check_pool_input(const torch::Tensor& x) {
  const bool f32 = x.scalar_type() == torch::kFloat;
  TORCH_CHECK(f32 || x.scalar_type() == torch::kHalf, "x must be fp16 or fp32");
  check_operand(x, "x", x.scalar_type(), 4, x.device());
  TORCH_CHECK(x.size(3) % (f32 ? 4 : 8) == 0, "x must be [B,H,W,C] with C % 8 (fp16) / 4 (fp32) == 0");
  return f32;
}

torch::Tensor maxpool2d_nhwc(torch::Tensor x, int64_t k, int64_t s, int64_t pad, c10::optional<torch::Tensor> out) {
  const bool f32 = check_pool_input(x);
  TORCH_CHECK(k >= 1 && s >= 1 && pad >= 0 && 2 * pad <= k, "bad pool geometry");
  const int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty output");
  auto y = optional_out(out, x.device(), x.scalar_type(), {B, Ho, Wo, C});
  if (!B) return y;
  if (f32) {
    maxpool_f32_launch(x.data_ptr<float>(), y.data_ptr<float>(), B, H, W, C, Ho, Wo, k, s, pad, cur_stream());
    check_launch("maxpool_f32");
    return y;
  }
  maxpool_launch(reinterpret_cast<const half_t*>(x.data_ptr()), reinterpret_cast<half_t*>(y.data_ptr()), B, H, W, C,
                 Ho, Wo, k, s, pad, cur_stream());
  check_launch("maxpool");
  return y;
}

torch::Tensor global_avgpool_nhwc(torch::Tensor x) {
  const bool f32 = check_pool_input(x);
  const int B = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  auto y = torch::empty({B, C}, x.options());
  if (!B) return y;
  if (f32) {
    avgpool_f32_launch(x.data_ptr<float>(), y.data_ptr<float>(), B, HW, C, cur_stream());
    check_launch("avgpool_f32");
    return y;
  }
  avgpool_launch(reinterpret_cast<const half_t*>(x.data_ptr()), reinterpret_cast<half_t*>(y.data_ptr()), B, HW, C,
                 cur_stream());
  check_launch("avgpool");
  return y;
}

// Optional `packed` [>= rows, 2] int32: also write (class, prob bits) pairs there
// (the data plane's gather send buffer, so no repack kernel runs afterwards).
std::vector<torch::Tensor> softmax_top1(torch::Tensor logits, c10::optional<torch::Tensor> packed,
                                        c10::optional<torch::Tensor> ovf) {
  const auto dev = logits.device();
  check_operand(logits, "logits", torch::kFloat, 2, dev, false);
  TORCH_CHECK(logits.stride(1) == 1, "logits must be [rows, N] with unit column stride");
  const int rows = logits.size(0), N = logits.size(1), ld = logits.stride(0);
  auto cls = torch::empty({rows}, logits.options().dtype(torch::kInt));
  auto prob = torch::empty({rows}, logits.options());
  int* pk = nullptr;
  if (packed.has_value() && packed->defined()) {
    check_operand(*packed, "packed", torch::kInt, 2, dev);
    TORCH_CHECK(packed->size(1) == 2 && packed->size(0) >= rows, "packed must be [>= rows, 2] int32");
    pk = packed->data_ptr<int>();
  }
  const int* of = nullptr;
  if (ovf.has_value() && ovf->defined()) {
    check_operand(*ovf, "ovf", torch::kInt, -1, dev, false);
    TORCH_CHECK(ovf->numel() >= 1, "ovf must be an int32 flag on the logits device");
    of = ovf->data_ptr<int>();
  }
  if (rows) softmax_top1_launch(logits.data_ptr<float>(), ld, N, rows, cls.data_ptr<int>(), prob.data_ptr<float>(),
                                pk, of, cur_stream());
  check_launch("softmax_top1");
  return {cls, prob};
}

// (cls int32 [rows, k], prob fp32 [rows, k]) of fp32 logits [rows, N] (row stride >= N, unit
// column stride): the k best classes of each row in stable descending order.
std::vector<torch::Tensor> softmax_topk(torch::Tensor logits, int64_t k, c10::optional<torch::Tensor> ovf) {
  const auto dev = logits.device();
  check_operand(logits, "logits", torch::kFloat, 2, dev, false);
  TORCH_CHECK(logits.stride(1) == 1, "logits must be [rows, N] with unit column stride");
  const int rows = logits.size(0), N = logits.size(1), ld = logits.stride(0);
  TORCH_CHECK(rows <= 1 || ld >= N, "logits rows must not overlap (row stride ", ld, " < N ", N, ")");
  TORCH_CHECK(k >= 1 && k <= 16 && k <= N, "k must be in [1, min(N, 16)], got k = ", k, " for N = ", N);
  auto cls = torch::empty({rows, k}, logits.options().dtype(torch::kInt));
  auto prob = torch::empty({rows, k}, logits.options());
  const int* of = nullptr;
  if (ovf.has_value() && ovf->defined()) {
    check_operand(*ovf, "ovf", torch::kInt, -1, dev, false);
    TORCH_CHECK(ovf->numel() >= 1, "ovf must be an int32 flag on the logits device");
    of = ovf->data_ptr<int>();
  }
  if (rows) softmax_topk_launch(logits.data_ptr<float>(), ld, N, rows, (int)k, cls.data_ptr<int>(),
                                prob.data_ptr<float>(), of, cur_stream());
  check_launch("softmax_topk");
  return {cls, prob};
}

// hipGraphLaunch of an instantiated graph (torch.cuda.CUDAGraph.raw_cuda_graph_exec())
// on the current stream, and nothing else: the round paths replay one graph per
// chunk and must not wait on the device in between (HipRunner._replayer).
void graph_launch(int64_t exec) {
  TORCH_CHECK(exec != 0, "graph_launch: no instantiated graph");
  const hipError_t e = hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(exec), cur_stream());
  TORCH_CHECK(e == hipSuccess, "hipGraphLaunch failed: ", hipGetErrorString(e));
}

torch::Tensor synth_images(int64_t seed, int64_t start, int64_t n, int64_t hw, torch::Device dev) {
  TORCH_CHECK(dev.is_cuda(), "synth_images needs a GPU device");
  TORCH_CHECK(n >= 0 && start >= 0 && (hw * hw * 3) % 8 == 0, "bad synth_images args");
  auto out = torch::empty({n, hw, hw, 3}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
  if (n) synth_images_launch(out.data_ptr<uint8_t>(), (uint64_t)seed, start, n, hw * hw * 3, cur_stream());
  check_launch("synth_images");
  return out;
}

int64_t pick_tile(int64_t M, int64_t Cout) { return conv_glds_pick((int)M, (int)Cout); }
int64_t pick_tile_split(int64_t M, int64_t Cout) { return conv_glds_split_pick((int)M, (int)Cout); }
int64_t pick_tile_f32(int64_t M, int64_t Cout, int64_t K, bool small) {
  return conv_f32_pick((int)M, (int)Cout, (int)K, small);
}
