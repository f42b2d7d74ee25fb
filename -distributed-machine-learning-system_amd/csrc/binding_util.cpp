// The one definition of everything binding_util.h declares (see its header comment).
#include "binding_util.h"

#include <mutex>

namespace idunno {

const int kRouteNoBand = 1, kRouteNoC64 = 2, kRouteNoStream1x1 = 4, kRouteLegacySmallM = 8, kRouteC64TwoPerCU = 16,
          kRouteBandW7 = 32, kRouteNoBandW28 = 64;

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

void check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, what, ": HIP launch failed: ", hipGetErrorString(e));
}

// The DMA source of padding taps / masked rows.  Created once per device under a
// lock and never freed: several node threads share one GPU, and a buffer replaced
// by a racing thread would go back to the caching allocator while kernels still
// read it as "zeros".
torch::Tensor zero_buffer(const torch::Device& dev) {
  static std::mutex mu;
  static std::vector<torch::Tensor>* bufs = new std::vector<torch::Tensor>(64);
  const int i = dev.index() < 0 ? 0 : dev.index();
  TORCH_CHECK(i < 64, "device index out of range");
  std::lock_guard<std::mutex> lk(mu);
  auto& b = (*bufs)[i];
  if (!b.defined()) {
    b = torch::zeros({256}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    // other threads' streams will read it: make the fill complete before publishing
    (void)hipStreamSynchronize(cur_stream());
  }
  return b;
}

// The bias of split-K partial GEMMs, grown on demand (same reasoning as zero_buffer).
torch::Tensor zero_f32(const torch::Device& dev, int64_t n) {
  static std::mutex mu;
  static std::vector<torch::Tensor>* bufs = new std::vector<torch::Tensor>(64);
  const int i = dev.index() < 0 ? 0 : dev.index();
  TORCH_CHECK(i < 64, "device index out of range");
  std::lock_guard<std::mutex> lk(mu);
  static std::vector<torch::Tensor>* retired = new std::vector<torch::Tensor>();
  auto& b = (*bufs)[i];
  if (!b.defined() || b.numel() < n) {
    // a smaller buffer may still be read by queued kernels (other threads'
    // streams, captured graphs): keep it alive instead of returning it to the
    // caching allocator, where it could be reused while "zero"
    if (b.defined()) retired->push_back(b);
    b = torch::zeros({std::max<int64_t>(n, 4096)}, torch::TensorOptions().dtype(torch::kFloat).device(dev));
    (void)hipStreamSynchronize(cur_stream());
  }
  return b;
}

// HipRunner sets the guard around a split forward (a captured graph keeps the pointer).
static thread_local int* g_split_guard = nullptr;
static thread_local int g_split_guard_dev = -1;
void set_split_guard(c10::optional<torch::Tensor> flag) {
  if (!flag.has_value() || !flag->defined()) {
    g_split_guard = nullptr;
    g_split_guard_dev = -1;
    return;
  }
  check_operand(*flag, "flag", torch::kInt, -1, flag->device());
  TORCH_CHECK(flag->numel() >= 1, "split guard flag must hold one int32");
  g_split_guard = flag->data_ptr<int>();
  g_split_guard_dev = flag->device().index();
}
int* split_guard_for(const torch::Device& dev) {
  if (g_split_guard == nullptr) return nullptr;
  TORCH_CHECK(dev.index() == g_split_guard_dev, "split guard flag lives on another device");
  return g_split_guard;
}

void check_operand(const torch::Tensor& t, const char* name, at::ScalarType dt, int rank, const torch::Device& dev,
                   bool contig) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.device() == dev, name, " is on a different device than the other operands");
  TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype");
  TORCH_CHECK(rank < 0 || t.dim() == rank, name, " must have rank ", rank);
  TORCH_CHECK(!contig || t.is_contiguous(), name, " must be contiguous");
}

int64_t nhwc_pixel_stride(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.dim() == 4, what, " must be 4-D NHWC");
  const int64_t P = t.stride(2);
  TORCH_CHECK(t.stride(3) == 1 && P >= t.size(3) && t.stride(1) == t.size(2) * P && t.stride(0) == t.size(1) * t.stride(1),
              what, " must be NHWC with contiguous channels and equally strided pixels");
  TORCH_CHECK(P % 8 == 0 && t.storage_offset() % 8 == 0, what, " pixel stride / offset must be 16-byte aligned");
  return P;
}

torch::Tensor optional_out(const c10::optional<torch::Tensor>& out, const torch::Device& dev, at::ScalarType dt,
                           at::IntArrayRef shape) {
  if (!out.has_value() || !out->defined()) return torch::empty(shape, torch::TensorOptions().dtype(dt).device(dev));
  check_operand(*out, "out", dt, (int)shape.size(), dev);
  TORCH_CHECK(out->sizes() == shape, "out shape mismatch: expected ", shape);
  return *out;
}

const void* optional_res(const c10::optional<torch::Tensor>& res, const torch::Device& dev, at::ScalarType dt,
                         at::IntArrayRef shape, int64_t* pixel_stride) {
  if (!res.has_value() || !res->defined()) return nullptr;
  check_operand(*res, "residual", dt, (int)shape.size(), dev, pixel_stride == nullptr);
  if (pixel_stride != nullptr) *pixel_stride = nhwc_pixel_stride(*res, "residual");
  TORCH_CHECK(res->sizes() == shape, "residual shape mismatch: expected ", shape);
  return res->data_ptr();
}

void check_strided_input(const torch::Tensor& x2, int B, int Ho, int Wo, int64_t stride) {
  TORCH_CHECK(stride >= 1, "bad stride");
  TORCH_CHECK(x2.size(0) == B && (x2.size(1) - 1) / stride + 1 == Ho && (x2.size(2) - 1) / stride + 1 == Wo,
              "x2 must be the block input at `stride` of x1's resolution");
}

// Packed-row geometry of an RGB stem (conv_f32 mode 2 / conv_glds pack3,
// preprocess_pack3): nc row copies (the distinct 16-byte phases of 3*stride*ox
// for E = 16 / elem_bytes elements per chunk), wp elements each, cpk 16-byte
// chunks per kernel row.
void pack3_geometry(int W, int KW, int stride, int pad, int elem_bytes, int& nc, int& wp, int& cpk) {
  const int E = 16 / elem_bytes;
  int g = 1;                                   // gcd(3 * stride, E), E a power of two
  while (g < E && (3 * stride) % (2 * g) == 0) g *= 2;
  nc = E / g;
  wp = (3 * (W + 2 * pad) + E - 1 + E - 1) / E * E;
  cpk = (3 * KW + E - 1) / E;
}

const long long* window_args(const torch::Tensor& img, const c10::optional<torch::Tensor>& start, int64_t batch,
                             int64_t window, int64_t sub, int& B, long long& max_start) {
  B = img.size(0);
  max_start = 0;
  if (!start.has_value() || !start->defined()) return nullptr;
  check_operand(*start, "start", torch::kLong, -1, img.device(), false);
  TORCH_CHECK(start->numel() == 1, "start must be a 1-element int64 tensor");
  TORCH_CHECK(batch > 0 && batch <= img.size(0), "window batch out of range");
  if (window <= 0) window = batch;
  TORCH_CHECK(window <= img.size(0) && sub >= 0 && sub + batch <= window, "window part out of range");
  B = (int)batch;
  max_start = img.size(0) - window;
  return reinterpret_cast<const long long*>(start->data_ptr());
}

}  // namespace idunno
