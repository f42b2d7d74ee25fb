// Python module table of the IDunno-MI355X HIP kernels.
//
// The entry points live in the bind_*.cpp families (declared below); every one
// validates the operand shapes/dtypes/devices it is handed with binding_util.h
// before it launches anything (a malformed launch on a shared MI355X box can
// fault the whole node), then launches on PyTorch's *current* HIP stream so
// the ops compose with torch.cuda.graph capture (hipGraph) and side streams.
#include "binding_util.h"

using torch::Tensor;
using OptTensor = c10::optional<torch::Tensor>;
using namespace idunno;

// bind_conv_f16.cpp
Tensor conv2d_nhwc(Tensor x, Tensor w, Tensor bias, OptTensor res, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                   bool relu, bool out_f32, int64_t tile, OptTensor out, int64_t ksplit, int64_t route);
Tensor conv1x1_dual(Tensor x1, Tensor x2, Tensor w, Tensor bias, int64_t stride, bool relu);
bool conv1x1_dual_ok(int64_t K1, int64_t K2, int64_t Cout, int64_t M);
std::vector<Tensor> conv1x1_fused_next(Tensor x1, OptTensor x2, Tensor w, Tensor bias, OptTensor res, Tensor w2,
                                       Tensor b2, int64_t stride, bool relu);
bool conv1x1_fused_next_ok(int64_t K1, int64_t K2, int64_t N, int64_t N2, int64_t M);
Tensor conv3x3_band_f16(Tensor x, Tensor w, Tensor bias, OptTensor res, bool relu, int64_t max_grid);
Tensor linear_splitk(Tensor x, Tensor w, Tensor bias, bool relu, bool out_f32, int64_t splits, int64_t tile);
// bind_conv_split.cpp
Tensor conv2d_split(Tensor x, Tensor w, Tensor bias, OptTensor res, int64_t KH, int64_t KW, int64_t stride,
                    int64_t pad, bool relu, double acc_scale, bool out_f32, int64_t tile, OptTensor out,
                    int64_t ksplit, int64_t route);
Tensor conv2d_split_dual(Tensor x, Tensor w, Tensor bias, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                         bool relu, double acc_scale, double acc_scale2, int64_t nsplit, bool center_only,
                         int64_t tile);
Tensor conv2d_split_tail(Tensor y, Tensor x2, Tensor w, Tensor bias, double acc_scale, int64_t stride2, bool relu,
                         int64_t tile);
bool conv2d_split_tail_ok(int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Cx, int64_t Cout, int64_t mode);
Tensor conv1x1_dual_split(Tensor x1, Tensor x2, Tensor w, Tensor bias, double acc_scale, int64_t stride, bool relu);
bool conv1x1_dual_split_ok(int64_t K1, int64_t K2, int64_t Cout, int64_t M);
Tensor conv3x3_band_split(Tensor x, Tensor w, Tensor bias, OptTensor res, bool relu, double acc_scale, bool out_f32,
                          int64_t max_grid, int64_t flags);
Tensor linear_split(Tensor x, Tensor w, Tensor bias, double acc_scale, bool relu, bool out_f32, int64_t splits,
                    int64_t tile);
Tensor split_from_f32(Tensor x);
Tensor f32_from_split(Tensor x);
Tensor maxpool2d_split(Tensor x, int64_t k, int64_t s, int64_t pad, OptTensor out);
// bind_conv_grouped.cpp
Tensor conv3x3_grouped(Tensor x, Tensor w, Tensor bias, int64_t groups, int64_t stride, bool relu);
Tensor conv3x3_grouped_split(Tensor x, Tensor w, Tensor bias, double acc_scale, int64_t groups, int64_t stride,
                             bool relu);
bool conv3x3_grouped_ok(int64_t C, int64_t groups, int64_t stride);
// bind_conv_f32.cpp
Tensor conv2d_nhwc_f32(Tensor x, Tensor w, Tensor bias, OptTensor res, int64_t KH, int64_t KW, int64_t stride,
                       int64_t pad, bool relu, int64_t tile, OptTensor out);
Tensor linear_f32_splitk(Tensor x, Tensor w, Tensor bias, bool relu, int64_t splits, int64_t tile);
Tensor conv2d_wino_f32(Tensor x, Tensor u, Tensor bias, OptTensor res, bool relu, int64_t variant);
Tensor conv2d_pack3(Tensor x3, Tensor w, Tensor bias, int64_t W, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                    bool relu, int64_t tile);
Tensor conv2d_pack3_split(Tensor x3, Tensor w, Tensor bias, int64_t W, int64_t KH, int64_t KW, int64_t stride,
                          int64_t pad, bool relu, double acc_scale, int64_t tile);
// bind_stem.cpp
Tensor stem_fused(Tensor img, Tensor w, Tensor bias, OptTensor start, int64_t batch, int64_t start_offset,
                  int64_t window, int64_t sub);
Tensor alex_stem_split(Tensor img, Tensor w, Tensor bias, Tensor psum, double acc_scale, OptTensor start,
                       int64_t batch, int64_t start_offset, int64_t window, int64_t sub, int64_t form);
Tensor alex_stem_u8_f16(Tensor img, Tensor w, Tensor bias, Tensor psum, double acc_scale, OptTensor start,
                        int64_t batch, int64_t start_offset, int64_t window, int64_t sub, int64_t form);
Tensor stem_split(Tensor img, Tensor w, Tensor bias, Tensor psum, double acc_scale, OptTensor start, int64_t batch,
                  int64_t start_offset, int64_t window, int64_t sub);
Tensor stem_u8_f16(Tensor img, Tensor w, Tensor bias, Tensor psum, double acc_scale, OptTensor start, int64_t batch,
                   int64_t start_offset, int64_t window, int64_t sub);
Tensor preprocess(Tensor img, OptTensor start, int64_t batch, int64_t start_offset, int64_t window, int64_t sub,
                  bool f32);
Tensor preprocess_pack3(Tensor img, int64_t KW, int64_t stride, int64_t pad, OptTensor start, int64_t batch,
                        int64_t start_offset, int64_t window, int64_t sub, bool f16);
Tensor preprocess_pack3_split(Tensor img, int64_t KW, int64_t stride, int64_t pad, OptTensor start, int64_t batch,
                              int64_t start_offset, int64_t window, int64_t sub);
std::tuple<int64_t, int64_t, int64_t, int64_t> resize_crop_geometry_py(int64_t Hi, int64_t Wi, int64_t resize,
                                                                       int64_t crop);
Tensor resize_crop(Tensor img, int64_t resize, int64_t crop);
// bind_elementwise.cpp
Tensor maxpool2d_nhwc(Tensor x, int64_t k, int64_t s, int64_t pad, OptTensor out);
Tensor global_avgpool_nhwc(Tensor x);
std::vector<Tensor> softmax_top1(Tensor logits, OptTensor packed, OptTensor ovf);
std::vector<Tensor> softmax_topk(Tensor logits, int64_t k, OptTensor ovf);
void graph_launch(int64_t exec);
Tensor synth_images(int64_t seed, int64_t start, int64_t n, int64_t hw, torch::Device dev);
int64_t pick_tile(int64_t M, int64_t Cout);
int64_t pick_tile_split(int64_t M, int64_t Cout);
int64_t pick_tile_f32(int64_t M, int64_t Cout, int64_t K, bool small);
// bind_jpeg.cpp: registers its own functions and classes (their types are complete only there)
void bind_jpeg(py::module_& m);
namespace idunno {   // runtime/staging.cpp
std::vector<double> stage_file_native(const std::string& path, Tensor out, std::vector<Tensor> pinned, int64_t stream,
                                      int64_t nthreads);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "IDunno-MI355X native HIP kernels (gfx950)";
  m.def("conv1x1_dual", &conv1x1_dual, "bottleneck expansion 1x1 + 1x1 downsample as one GEMM (fp16)",
        py::arg("x1"), py::arg("x2"), py::arg("w"), py::arg("bias"), py::arg("stride"), py::arg("relu"));
  m.def("conv1x1_dual_ok", &conv1x1_dual_ok, "whether conv1x1_dual supports (K1, K2, Cout, M)");
  m.def("conv1x1_fused_next", &conv1x1_fused_next, "bottleneck tail + next block's reduce 1x1 in one pass (fp16)",
        py::arg("x1"), py::arg("x2"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("w2"), py::arg("b2"),
        py::arg("stride"), py::arg("relu"));
  m.def("conv1x1_fused_next_ok", &conv1x1_fused_next_ok, "whether conv1x1_fused_next supports (K1, K2, N, N2, M)");
  m.def("conv1x1_dual_split", &conv1x1_dual_split, "split (fp32-accurate) form of conv1x1_dual", py::arg("x1"),
        py::arg("x2"), py::arg("w"), py::arg("bias"), py::arg("acc_scale"), py::arg("stride"), py::arg("relu"));
  m.def("conv1x1_dual_split_ok", &conv1x1_dual_split_ok, "whether conv1x1_dual_split supports (K1, K2, Cout, M)");
  m.def("conv2d_nhwc", &conv2d_nhwc, "implicit-GEMM MFMA conv + bias (+res) (+relu)", py::arg("x"), py::arg("w"),
        py::arg("bias"), py::arg("res"), py::arg("KH"), py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("relu"), py::arg("out_f32") = false, py::arg("tile") = -1, py::arg("out") = py::none(),
        py::arg("ksplit") = -1, py::arg("route") = 0);
  m.def("linear_splitk", &linear_splitk, "FC layer with split-K partial GEMMs + combine", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("relu"), py::arg("out_f32"), py::arg("splits"), py::arg("tile") = -1);
  m.def("conv2d_split", &conv2d_split, "split-fp16 (fp32-accurate) conv: 3 f16 MFMAs per 32 channels",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
        py::arg("pad"), py::arg("relu"), py::arg("acc_scale"), py::arg("out_f32") = false, py::arg("tile") = -1,
        py::arg("out") = py::none(), py::arg("ksplit") = -1, py::arg("route") = 0);
  m.def("conv2d_split_dual", &conv2d_split_dual,
        "two split convs of one input in one launch (downsample as the centre tap of the 3x3/s conv)",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("KH"), py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("relu"), py::arg("acc_scale"), py::arg("acc_scale2"), py::arg("nsplit"), py::arg("center_only"),
        py::arg("tile") = -1);
  m.def("conv2d_split_tail", &conv2d_split_tail,
        "split 3x3/s1/p1 conv of y + 1x1/stride2 conv of x2 as one GEMM over the concatenated K (block tail + downsample)",
        py::arg("y"), py::arg("x2"), py::arg("w"), py::arg("bias"), py::arg("acc_scale"), py::arg("stride2"),
        py::arg("relu"), py::arg("tile") = -1);
  m.def("conv2d_split_tail_ok", &conv2d_split_tail_ok,
        "whether the K-tail fusion is the default for (B, Ho, Wo, C, Cx, Cout); mode 2: wherever supported, 3: not over the band kernel",
        py::arg("B"), py::arg("Ho"), py::arg("Wo"), py::arg("C"), py::arg("Cx"), py::arg("Cout"), py::arg("mode") = 1);
  m.def("conv2d_pack3_split", &conv2d_pack3_split, "split-fp16 RGB stem conv on packed rows, fp32 out",
        py::arg("x3"), py::arg("w"), py::arg("bias"), py::arg("W"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
        py::arg("pad"), py::arg("relu"), py::arg("acc_scale"), py::arg("tile") = -1);
  m.def("preprocess_pack3_split", &preprocess_pack3_split, "uint8 HWC -> split-fp16 packed-row stem input",
        py::arg("img"), py::arg("KW"), py::arg("stride"), py::arg("pad"), py::arg("start") = py::none(),
        py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1, py::arg("sub") = 0);
  m.def("stem_u8_f16", &stem_u8_f16, "fp16 fused ResNet stem in exact-u8 form (pack_stem_split weights)",
        py::arg("img"), py::arg("w"), py::arg("bias"), py::arg("psum"), py::arg("acc_scale"), py::arg("start") = py::none(),
        py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1, py::arg("sub") = 0);
  m.def("stem_split", &stem_split, "fp32-accurate fused split-fp16 ResNet stem (normalise+conv7x7/2+relu+maxpool)",
        py::arg("img"), py::arg("w"), py::arg("bias"), py::arg("psum"), py::arg("acc_scale"), py::arg("start") = py::none(),
        py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1, py::arg("sub") = 0);
  m.def("linear_split", &linear_split, "fp32-accurate FC on split fp16, split-K in one launch + combine",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("acc_scale"), py::arg("relu"), py::arg("out_f32"),
        py::arg("splits"), py::arg("tile") = -1);
  m.def("conv3x3_band_split", &conv3x3_band_split,
        "band-staged split 3x3/s1/p1 conv (tile 70) with a persistent-grid cap (0: one workgroup per CU)",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res") = py::none(), py::arg("relu") = true,
        py::arg("acc_scale") = 1.0, py::arg("out_f32") = false, py::arg("max_grid") = 0, py::arg("flags") = 0);
  m.def("conv3x3_band_f16", &conv3x3_band_f16,
        "band-staged fp16 3x3/s1/p1 conv (tile 70) with a persistent-grid cap (0: one workgroup per CU)",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("relu"), py::arg("max_grid") = 0);
  m.def("conv3x3_band_tiles", &conv3x3_band_tiles, "band conv tile count for (B, W, Cout)");
  m.def("split_from_f32", &split_from_f32, "fp32 NHWC -> split-fp16 layout");
  m.def("f32_from_split", &f32_from_split, "split-fp16 layout -> fp32 NHWC");
  m.def("maxpool2d_split", &maxpool2d_split, "NHWC max pool (fp32 or split in) -> split out", py::arg("x"),
        py::arg("k"), py::arg("s"), py::arg("pad"), py::arg("out") = py::none());
  m.def("alex_stem_u8_f16", &alex_stem_u8_f16,
        "fp16 fused AlexNet stem (exact-u8 form, hi MFMA only); form: -1 default, 0 one-half workgroups, 1 phased",
        py::arg("img"), py::arg("w"), py::arg("bias"), py::arg("psum"), py::arg("acc_scale"),
        py::arg("start") = py::none(), py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1,
        py::arg("sub") = 0, py::arg("form") = -1);
  m.def("alex_stem_split", &alex_stem_split,
        "fused split AlexNet stem (conv 11x11/4 + ReLU + max pool 3x3/2); form: -1 default, 0 one-half workgroups, 1 phased",
        py::arg("img"), py::arg("w"), py::arg("bias"), py::arg("psum"), py::arg("acc_scale"),
        py::arg("start") = py::none(), py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1,
        py::arg("sub") = 0, py::arg("form") = -1);
  m.def("conv3x3_grouped", &conv3x3_grouped, "grouped 3x3 pad-1 conv + bias (+relu), fp16 NHWC", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("groups"), py::arg("stride"), py::arg("relu"));
  m.def("conv3x3_grouped_split", &conv3x3_grouped_split,
        "grouped 3x3 pad-1 conv + bias (+relu) on split-fp16 operands (fp32-accurate, range-guarded)", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("acc_scale"), py::arg("groups"), py::arg("stride"), py::arg("relu"));
  m.def("conv3x3_grouped_ok", &conv3x3_grouped_ok, "whether the grouped 3x3 kernel takes (C, groups, stride)");
  m.def("pick_tile_split", &pick_tile_split, "split conv tile heuristic for (M, Cout)");
  m.def("conv2d_nhwc_f32", &conv2d_nhwc_f32, "fp32 implicit-GEMM conv on f32 MFMA + bias (+res) (+relu)",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
        py::arg("pad"), py::arg("relu"), py::arg("tile") = -1, py::arg("out") = py::none());
  m.def("linear_f32_splitk", &linear_f32_splitk, "fp32 FC with split-K in one launch + combine", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("relu"), py::arg("splits"), py::arg("tile") = -1);
  m.def("conv2d_pack3", &conv2d_pack3, "RGB stem conv on packed rows (preprocess_pack3), fp32 or fp16 + bias (+relu)",
        py::arg("x3"), py::arg("w"), py::arg("bias"), py::arg("W"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
        py::arg("pad"), py::arg("relu"), py::arg("tile") = -1);
  m.def("preprocess_pack3", &preprocess_pack3, "uint8 HWC -> packed-row fp32 stem input [B, H, nc, wp]",
        py::arg("img"), py::arg("KW"), py::arg("stride"), py::arg("pad"), py::arg("start") = py::none(),
        py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1, py::arg("sub") = 0,
        py::arg("f16") = false);
  m.def("conv2d_wino_f32", &conv2d_wino_f32, "fp32 Winograd F(2x2,3x3) conv (3x3/s1/p1) + bias (+res) (+relu)",
        py::arg("x"), py::arg("u"), py::arg("bias"), py::arg("res"), py::arg("relu"), py::arg("variant") = 0);
  m.def("wino_supported", &conv_wino_f32_supported, "winograd conv geometry fits (H, W, C, Cout)");
  m.def("pick_tile_f32", &pick_tile_f32, "tile id the f32 conv heuristic picks for (M, Cout, K, small)");
  m.def("preprocess", &preprocess, "uint8 HWC -> normalised fp16 (or fp32) NHWC4", py::arg("img"),
        py::arg("start") = py::none(), py::arg("batch") = -1, py::arg("start_offset") = 0, py::arg("window") = -1,
        py::arg("sub") = 0, py::arg("f32") = false);
  m.def("stem_fused", &stem_fused, "fused normalise + conv7x7/2 + bias + relu + maxpool3x3/2 (ResNet stem)",
        py::arg("img"), py::arg("w"), py::arg("bias"), py::arg("start") = py::none(), py::arg("batch") = -1,
        py::arg("start_offset") = 0, py::arg("window") = -1, py::arg("sub") = 0);
  m.def("resize_crop", &resize_crop, "bilinear resize + centre crop + normalise");
  m.def("resize_crop_geometry", &resize_crop_geometry_py,
        "host only: (Hr, Wr, top, left) of resize_crop on an Hi x Wi image", py::arg("Hi"), py::arg("Wi"),
        py::arg("resize"), py::arg("crop"));
  m.def("maxpool2d_nhwc", &maxpool2d_nhwc, "NHWC max pool (into ``out`` when given)", py::arg("x"), py::arg("k"),
        py::arg("s"), py::arg("pad"), py::arg("out") = py::none());
  m.def("global_avgpool_nhwc", &global_avgpool_nhwc, "NHWC global average pool");
  m.def("softmax_top1", &softmax_top1, "fused row softmax + argmax; a set ``ovf`` flag marks every row -2",
        py::arg("logits"), py::arg("packed") = py::none(), py::arg("ovf") = py::none());
  m.def("softmax_topk", &softmax_topk,
        "fused row softmax + the k best classes in stable descending order; a set ``ovf`` flag marks every entry -2",
        py::arg("logits"), py::arg("k"), py::arg("ovf") = py::none());
  m.def("set_split_guard", &set_split_guard,
        "split range guard flag (int32 device tensor) for this thread's split launches; None = off",
        py::arg("flag") = py::none());
  m.def("synth_images", &synth_images, "deterministic synthetic uint8 images [n,hw,hw,3]");
  m.def("stage_file_native", &idunno::stage_file_native,
        "host -> HBM staging of a file's bytes into `out` through pinned ping-pong buffers on `stream`, "
        "parallel pread(2) with the GIL released (runtime/staging.cpp)",
        py::arg("path"), py::arg("out"), py::arg("pinned"), py::arg("stream"), py::arg("nthreads") = 8);
  bind_jpeg(m);
  m.def("graph_launch", &graph_launch, "hipGraphLaunch(exec, current stream): a replay without any host wait");
  m.def("pick_tile", &pick_tile, "tile id the conv heuristic picks for (M, Cout)");
}
