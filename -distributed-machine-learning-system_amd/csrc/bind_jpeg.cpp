// JPEG source: host entropy decode, the device entropy stage, GPU IDCT / resize (runtime/jpeg.py).
#include "binding_util.h"
#include "runtime/jpeg_entropy.h"
#include "runtime/jpeg_huff_pack.h"

using namespace idunno;

// ---- JPEG source: host entropy decode + GPU IDCT / resize (runtime/jpeg.py) ----
static py::dict jpeg_header_dict(const JpegHeader& h) {
  py::dict d;
  d["W"] = h.W;
  d["H"] = h.H;
  d["ncomp"] = h.ncomp;
  d["hmax"] = h.hmax;
  d["vmax"] = h.vmax;
  d["mode"] = h.mode;
  d["restart_interval"] = h.restart_interval;
  d["total_coefs"] = (int64_t)h.total_coefs;
  d["progressive"] = h.progressive != 0;
  d["nscans"] = h.nscans;
  d["colorspace"] = h.colorspace;
  py::list comps;
  for (int c = 0; c < h.ncomp; ++c) {
    const JpegComp& cp = h.at(c);
    py::dict e;
    e["h"] = cp.h;
    e["v"] = cp.v;
    e["bw"] = cp.bw;
    e["bh"] = cp.bh;
    e["coef_off"] = (int64_t)cp.coef_off;
    e["q"] = std::vector<int>(cp.q, cp.q + 64);
    comps.append(e);
  }
  d["comp"] = comps;
  return d;
}

static void bytes_span(const py::handle& o, const uint8_t** p, size_t* n) {
  char* buf = nullptr;
  Py_ssize_t len = 0;
  TORCH_CHECK(PyBytes_Check(o.ptr()) && PyBytes_AsStringAndSize(o.ptr(), &buf, &len) == 0, "expected bytes");
  *p = reinterpret_cast<const uint8_t*>(buf);
  *n = (size_t)len;
}

// A list of bytes / None as pointers and lengths: nullptr / 0 for None and for empty bytes.
static void bytes_list(const py::list& datas, std::vector<const uint8_t*>* ptr, std::vector<size_t>* len) {
  const size_t n = datas.size();
  ptr->assign(n, nullptr);
  len->assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    py::handle o = datas[i];
    if (!o.is_none()) bytes_span(o, &(*ptr)[i], &(*len)[i]);
    if ((*len)[i] == 0) (*ptr)[i] = nullptr;
  }
}

// The flags of the Python functions below are the members of JpegOptions (runtime/jpeg_entropy.h),
// which says what each admits; the struct is built here and nowhere else.

// (status, reason, header dict or None)
py::tuple jpeg_parse(py::bytes data, bool native_progressive, bool native_sampling, bool native_colorspace) {
  JpegOptions opt;
  opt.native_progressive = native_progressive;
  opt.native_sampling = native_sampling;
  opt.native_colorspace = native_colorspace;
  const uint8_t* p;
  size_t n;
  bytes_span(data, &p, &n);
  JpegHeader h;
  const int st = jpeg_parse_header(n ? p : nullptr, n, &h, opt);
  return py::make_tuple(st, jpeg_status_name(st), st == JPEG_OK ? py::object(jpeg_header_dict(h)) : py::none());
}

// Entropy-decodes a list of bytes / None on `threads` native threads with the GIL
// released.  Returns (status per entry, headers uint8 [n, sizeof(JpegHeader)],
// coefficients int16 [total] on the host, first coefficient of each entry or -1).
// Only entries whose header parses get room in the coefficient buffer.
py::tuple jpeg_entropy_batch(py::list datas, int64_t threads, bool native_progressive, bool native_sampling,
                             bool native_colorspace) {
  JpegOptions opt;
  opt.native_progressive = native_progressive;
  opt.native_sampling = native_sampling;
  opt.native_colorspace = native_colorspace;
  const int n = (int)datas.size();
  TORCH_CHECK(threads >= 1 && threads <= 256, "threads out of range");
  std::vector<const uint8_t*> ptr;
  std::vector<size_t> len, cap(n, 0);
  bytes_list(datas, &ptr, &len);
  auto hdr = torch::zeros({n, (int64_t)sizeof(JpegHeader)}, torch::kUInt8);
  JpegHeader* hp = reinterpret_cast<JpegHeader*>(hdr.data_ptr());
  std::vector<int> status(n, JPEG_EMPTY);
  std::vector<int64_t> offs(n, -1);
  int64_t total = 0;
  {
    // sizes come from the headers alone (a few hundred marker bytes per file; the decode below
    // parses them again because it also needs the Huffman tables, which a header does not keep)
    py::gil_scoped_release nogil;
    for (int i = 0; i < n; ++i) {
      if (ptr[i] == nullptr) continue;
      status[i] = jpeg_parse_header(ptr[i], len[i], &hp[i], opt);
      if (status[i] != JPEG_OK) {
        ptr[i] = nullptr;                    // keeps its parse status: not decoded
        continue;
      }
      offs[i] = total;
      cap[i] = hp[i].total_coefs;
      total += (int64_t)hp[i].total_coefs;
    }
  }
  auto coefs = torch::empty({total}, torch::kInt16);
  int16_t* cp = total ? coefs.data_ptr<int16_t>() : nullptr;
  std::vector<int16_t*> out(n, nullptr);
  for (int i = 0; i < n; ++i)
    if (offs[i] >= 0) out[i] = cp + offs[i];
  {
    std::vector<int> st2(n, JPEG_EMPTY);
    std::vector<JpegHeader> h2((size_t)n);
    py::gil_scoped_release nogil;
    jpeg_decode_batch(n, ptr.data(), len.data(), h2.data(), out.data(), cap.data(), st2.data(), (int)threads, opt);
    for (int i = 0; i < n; ++i)
      if (ptr[i] != nullptr) status[i] = st2[i];
  }
  return py::make_tuple(status, hdr, coefs, offs);
}

// A validated batch: device descriptor tables and the buffer sizes the two kernels need.
struct JpegPlan {
  torch::Tensor desc, segs;          // device
  int64_t n_gpu = 0, nseg = 0, nblocks = 0, coef_elems = 0, plane_bytes = 0, out_bytes = 0, max_pix = 0;
  int64_t n_exact = 0;               // of the n_gpu images, those of mode 3 / 4 or RGB / CMYK / YCCK: their planes get the fp64 IDCT pass
  int64_t n_color = 0;               // of the n_gpu images, those with colorspace != 0: the resize kernel with their colour stages
  std::vector<int64_t> out_off;      // per entry: byte offset of its pixels in the output, -1: not on the GPU
  bool full_res = false;
};

// hdr, status, offs: what jpeg_entropy_batch returned; coef_elems: elements of its
// coefficient buffer.  geom int64 CPU [n, 4] = (rw, rh, left, top) per entry with
// a crop x crop output per entry, or None: full resolution, outputs back to back.
std::shared_ptr<JpegPlan> jpeg_plan(torch::Tensor hdr, std::vector<int64_t> status, std::vector<int64_t> offs,
                                    int64_t coef_elems, c10::optional<torch::Tensor> geom, int64_t crop,
                                    torch::Device dev) {
  TORCH_CHECK(dev.is_cuda(), "jpeg_plan needs a GPU device");
  const int64_t n = (int64_t)status.size();
  TORCH_CHECK(!hdr.is_cuda() && hdr.is_contiguous() && hdr.scalar_type() == torch::kUInt8 && hdr.dim() == 2 &&
                  hdr.size(0) == n && hdr.size(1) == (int64_t)sizeof(JpegHeader) && (int64_t)offs.size() == n,
              "jpeg_plan: headers / status / offsets do not match");
  const int64_t* gp = nullptr;
  if (geom.has_value()) {
    const auto& g = *geom;
    TORCH_CHECK(!g.is_cuda() && g.is_contiguous() && g.scalar_type() == torch::kLong && g.dim() == 2 &&
                    g.size(0) == n && g.size(1) == 4, "geom must be int64 CPU [n, 4]");
    TORCH_CHECK(crop >= 1 && crop <= kJpegMaxDim, "crop out of range");
    gp = g.data_ptr<int64_t>();
  }
  const JpegHeader* hp = reinterpret_cast<const JpegHeader*>(hdr.data_ptr());
  auto plan = std::make_shared<JpegPlan>();
  plan->full_res = gp == nullptr;
  plan->coef_elems = coef_elems;
  plan->out_off.assign(n, -1);
  std::vector<JpegImageDesc> descs;
  std::vector<JpegSeg> segs;
  int64_t planes = 0, outb = 0, nblocks = 0, max_pix = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (status[i] != JPEG_OK) continue;
    const JpegHeader& h = hp[i];
    // the layout is re-derived from the frame's size and sampling; a header that disagrees is refused
    TORCH_CHECK(h.W >= 1 && h.W <= kJpegMaxDim && h.H >= 1 && h.H <= kJpegMaxDim &&
                    (h.ncomp == 1 || h.ncomp == 3 || h.ncomp == 4) && h.mode >= 0 && h.mode <= 4, "jpeg_plan: bad header ", i);
    // grey: 0; three components: YCbCr or RGB; four: CMYK or YCCK, every plane full size
    TORCH_CHECK(h.ncomp == 1 ? h.colorspace == 0 : h.ncomp == 3 ? (h.colorspace == 0 || h.colorspace == 1)
                                                                : ((h.colorspace == 2 || h.colorspace == 3) && h.mode == 0),
                "jpeg_plan: bad colour space ", i);
    const int hmax = h.comp[0].h, vmax = h.comp[0].v;
    TORCH_CHECK(hmax >= 1 && hmax <= 4 && vmax >= 1 && vmax <= 4, "jpeg_plan: bad sampling ", i);
    const int mcux = (h.W + 8 * hmax - 1) / (8 * hmax), mcuy = (h.H + 8 * vmax - 1) / (8 * vmax);
    TORCH_CHECK(offs[i] >= 0 && offs[i] % 64 == 0 && offs[i] + (int64_t)h.total_coefs <= coef_elems,
                "jpeg_plan: coefficients of entry ", i, " outside the buffer");
    JpegImageDesc d;
    std::memset(&d, 0, sizeof(d));
    int64_t co = 0;
    for (int c = 0; c < h.ncomp; ++c) {
      const JpegComp& cp = h.at(c);
      TORCH_CHECK(cp.h >= 1 && cp.h <= hmax && cp.v >= 1 && cp.v <= vmax && hmax % cp.h == 0 && vmax % cp.v == 0 &&
                      cp.bw == mcux * cp.h && cp.bh == mcuy * cp.v && (int64_t)cp.coef_off == co,
                  "jpeg_plan: bad component layout ", i);
      if (c > 0) {
        const int fx = hmax / cp.h, fy = vmax / cp.v;
        TORCH_CHECK((h.mode == 0 && fx == 1 && fy == 1) || (h.mode == 1 && fx == 2 && fy == 1) ||
                        (h.mode == 2 && fx == 2 && fy == 2) || (h.mode == 3 && fx == 1 && fy == 2) ||
                        (h.mode == 4 && fx == 4 && fy == 1), "jpeg_plan: sampling mode mismatch ", i);
      }
      std::memcpy(d.q[c], cp.q, sizeof(cp.q));
      d.blk_off[c] = (int)((offs[i] + co) / 64);
      d.bw[c] = cp.bw;
      d.bh[c] = cp.bh;
      d.cw[c] = (h.W * cp.h + hmax - 1) / hmax;
      d.ch[c] = (h.H * cp.v + vmax - 1) / vmax;
      TORCH_CHECK(d.cw[c] <= 8 * cp.bw && d.ch[c] <= 8 * cp.bh && 8 * cp.bw <= 16 * ((cp.bw + 1) / 2), "jpeg_plan: plane smaller than its image ", i);
      const int bwp = (cp.bw + 1) / 2;              // pairs of blocks per block row
      d.pitch[c] = 16 * bwp;
      d.plane_off[c] = planes;
      planes += (int64_t)d.pitch[c] * cp.bh * 8;
      segs.push_back(JpegSeg{(int)(nblocks / 2), (int)descs.size(), c, 0});
      nblocks += 2 * (int64_t)bwp * cp.bh;         // block slots: two per pair
      co += (int64_t)cp.bw * cp.bh * 64;
    }
    TORCH_CHECK(co == (int64_t)h.total_coefs, "jpeg_plan: coefficient count mismatch ", i);
    d.W = h.W;
    d.H = h.H;
    d.ncomp = h.ncomp;
    d.mode = h.ncomp == 3 ? h.mode : 0;
    d.colorspace = h.colorspace;
    if (d.mode >= 3 || d.colorspace != 0) ++plan->n_exact;
    if (d.colorspace != 0) ++plan->n_color;
    if (gp != nullptr) {
      const int64_t rw = gp[4 * i], rh = gp[4 * i + 1], left = gp[4 * i + 2], top = gp[4 * i + 3];
      TORCH_CHECK(rw >= 1 && rw <= (1 << 16) && rh >= 1 && rh <= (1 << 16) && left >= -(1 << 16) &&
                      left <= (1 << 16) && top >= -(1 << 16) && top <= (1 << 16), "jpeg_plan: bad geometry ", i);
      d.rw = (int)rw;
      d.rh = (int)rh;
      d.left = (int)left;
      d.top = (int)top;
      d.out_w = d.out_h = (int)crop;
      d.out_off = i * crop * crop * 3;
      outb = n * crop * crop * 3;
    } else {
      d.rw = h.W;
      d.rh = h.H;
      d.out_w = h.W;
      d.out_h = h.H;
      d.out_off = outb;
      outb += (int64_t)h.W * h.H * 3;
    }
    plan->out_off[i] = d.out_off;
    max_pix = std::max<int64_t>(max_pix, (int64_t)d.out_w * d.out_h);
    descs.push_back(d);
  }
  // segments number the block pairs of the entries decoded here; each finds its coefficients through blk_off
  TORCH_CHECK(nblocks < (1ll << 31) / 64 * 64 && (int64_t)descs.size() <= 65535, "jpeg_plan: batch too large");
  plan->n_gpu = (int64_t)descs.size();
  plan->nseg = (int64_t)segs.size();
  plan->nblocks = nblocks;
  plan->plane_bytes = planes;
  plan->out_bytes = outb;
  plan->max_pix = max_pix;
  if (plan->n_gpu) {
    auto dt = torch::empty({(int64_t)(descs.size() * sizeof(JpegImageDesc))}, torch::kUInt8);
    std::memcpy(dt.data_ptr(), descs.data(), descs.size() * sizeof(JpegImageDesc));
    auto sgt = torch::empty({(int64_t)(segs.size() * sizeof(JpegSeg))}, torch::kUInt8);
    std::memcpy(sgt.data_ptr(), segs.data(), segs.size() * sizeof(JpegSeg));
    plan->desc = dt.to(dev);
    plan->segs = sgt.to(dev);
  }
  return plan;
}

void jpeg_idct(const std::shared_ptr<JpegPlan>& plan, torch::Tensor coefs, torch::Tensor planes) {
  TORCH_CHECK(plan != nullptr, "no plan");
  if (plan->n_gpu == 0) return;
  check_operand(coefs, "coefs", torch::kInt16, -1, plan->desc.device());
  check_operand(planes, "planes", torch::kUInt8, -1, plan->desc.device());
  TORCH_CHECK(coefs.numel() >= plan->coef_elems && planes.numel() >= plan->plane_bytes, "jpeg_idct: buffer too small");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(coefs.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(planes.data_ptr()) % 16 == 0, "jpeg_idct: buffers must be 16-byte aligned");
  jpeg_idct_launch(coefs.data_ptr<int16_t>(), planes.data_ptr<uint8_t>(),
                   reinterpret_cast<const JpegImageDesc*>(plan->desc.data_ptr()),
                   reinterpret_cast<const JpegSeg*>(plan->segs.data_ptr()), (int)plan->nseg, (int)plan->nblocks,
                   cur_stream());
  check_launch("jpeg_idct");
  if (plan->n_exact) {
    jpeg_idct_exact_launch(coefs.data_ptr<int16_t>(), planes.data_ptr<uint8_t>(),
                           reinterpret_cast<const JpegImageDesc*>(plan->desc.data_ptr()),
                           reinterpret_cast<const JpegSeg*>(plan->segs.data_ptr()), (int)plan->nseg, (int)plan->nblocks,
                           cur_stream());
    check_launch("jpeg_idct_exact");
  }
}

void jpeg_resize_crop(const std::shared_ptr<JpegPlan>& plan, torch::Tensor planes, torch::Tensor out) {
  TORCH_CHECK(plan != nullptr, "no plan");
  if (plan->n_gpu == 0) return;
  check_operand(planes, "planes", torch::kUInt8, -1, plan->desc.device());
  check_operand(out, "out", torch::kUInt8, -1, plan->desc.device());
  TORCH_CHECK(planes.numel() >= plan->plane_bytes && out.numel() >= plan->out_bytes,
              "jpeg_resize_crop: buffer too small");
  jpeg_resize_crop_launch(planes.data_ptr<uint8_t>(), reinterpret_cast<const JpegImageDesc*>(plan->desc.data_ptr()),
                          out.data_ptr<uint8_t>(), (int)plan->n_gpu, (int)plan->max_pix, plan->n_color != 0, cur_stream());
  check_launch("jpeg_resize_crop");
}

// ---- JPEG entropy stage on the device (runtime/jpeg_huff_pack.cpp, kernels/jpeg_entropy.hip) ----
// A parsed and packed batch, all on the host: what jpeg_entropy_batch returns minus the
// coefficients, plus the three buffers the entropy kernel reads.
struct JpegHuffPacked {
  std::vector<int64_t> status;       // per entry: the header parse's verdict (the kernel's comes later)
  std::vector<int64_t> offs;         // first coefficient of each accepted entry, else -1
  torch::Tensor hdr;                 // uint8 [n, sizeof(JpegHeader)]
  torch::Tensor bytes, sets, desc;   // uint8: entropy-coded bytes, JpegHuffSet[], JpegHuffDesc[n]
  int64_t n = 0, n_gpu = 0, nsets = 0, byte_total = 0, coef_total = 0;
  // packed for the sub-stream kernel (jpeg_huff_par.h): JpegParDesc[n], the entries it takes (gpu == 2),
  // those left to the one-lane kernel (restart markers) and the uint32 elements of scratch it needs
  bool parallel = false;
  torch::Tensor par;
  int64_t n_par = 0, n_lane = 0, scratch_total = 0;
  // what the batch was packed with; the checks before a launch admit what it admits
  JpegOptions opt;
  // the progressive entries (gpu == 3) as JpegProgScan[nscans], JpegHuffTab[ntabs] and the int32 indices
  // of those entries, for jpeg_entropy_prog_kernel
  torch::Tensor scans, tabs, prog_list;
  int64_t n_prog = 0, nscans = 0, ntabs = 0;
  // the baseline entries with a restart interval whose markers the packer found (gpu == 4) as
  // JpegRstItem[nitems], int32 [nitems, 4] = (entry, byte_begin, mcu_first, index), for
  // jpeg_entropy_rst_kernel; n_lane keeps counting the gpu == 1 entries only
  torch::Tensor rst_items;
  int64_t n_rst = 0;
};

// Parses a list of bytes / None and packs the accepted entries, GIL released.  parallel: lay the
// entries without restart markers out for the sub-stream kernel (jpeg_entropy_gpu_parallel).
std::shared_ptr<JpegHuffPacked> jpeg_huff_pack(py::list datas, bool parallel, bool native_progressive,
                                               bool restart_intervals, bool native_sampling, bool native_colorspace) {
  JpegOptions opt;
  opt.native_progressive = native_progressive;
  opt.restart_intervals = restart_intervals;
  opt.native_sampling = native_sampling;
  opt.native_colorspace = native_colorspace;
  const int n = (int)datas.size();
  std::vector<const uint8_t*> ptr;
  std::vector<size_t> len;
  bytes_list(datas, &ptr, &len);
  auto pk = std::make_shared<JpegHuffPacked>();
  pk->n = n;
  pk->hdr = torch::zeros({n, (int64_t)sizeof(JpegHeader)}, torch::kUInt8);
  std::vector<int> status(n, JPEG_EMPTY);
  JpegHuffBatch b;
  {
    py::gil_scoped_release nogil;
    jpeg_huff_plan(n, ptr.data(), len.data(), reinterpret_cast<JpegHeader*>(pk->hdr.data_ptr()), status.data(), &b,
                   parallel ? kJpegParSubBits : 0u, opt);
  }
  const char* why = parallel ? jpeg_huff_par_check(b.desc.data(), b.par.data(), n, b.byte_total, (int64_t)b.sets.size(),
                                                   b.coef_total, b.scratch_total, kJpegParSubBits, opt)
                             : jpeg_huff_check(b.desc.data(), n, b.byte_total, (int64_t)b.sets.size(), b.coef_total, opt);
  if (why == nullptr && opt.native_progressive)
    why = jpeg_huff_prog_check(b.desc.data(), n, b.scans.data(), (int64_t)b.scans.size(), (int64_t)b.tabs.size());
  if (why == nullptr) why = jpeg_huff_rst_check(b.desc.data(), n, b.rst_items.data(), (int64_t)b.rst_items.size());
  TORCH_CHECK(why == nullptr, "jpeg_huff_pack: bad descriptor: ", why ? why : "");
  pk->bytes = torch::empty({b.byte_total}, torch::kUInt8);
  pk->sets = torch::empty({(int64_t)(b.sets.size() * sizeof(JpegHuffSet))}, torch::kUInt8);
  pk->desc = torch::empty({(int64_t)(b.desc.size() * sizeof(JpegHuffDesc))}, torch::kUInt8);
  pk->parallel = parallel;
  pk->par = torch::empty({(int64_t)(b.par.size() * sizeof(JpegParDesc))}, torch::kUInt8);
  if (!b.par.empty()) std::memcpy(pk->par.data_ptr(), b.par.data(), b.par.size() * sizeof(JpegParDesc));
  pk->scratch_total = b.scratch_total;
  pk->opt = opt;
  pk->nscans = (int64_t)b.scans.size();
  pk->ntabs = (int64_t)b.tabs.size();
  pk->scans = torch::empty({(int64_t)(b.scans.size() * sizeof(JpegProgScan))}, torch::kUInt8);
  pk->tabs = torch::empty({(int64_t)(b.tabs.size() * sizeof(JpegHuffTab))}, torch::kUInt8);
  if (!b.scans.empty()) std::memcpy(pk->scans.data_ptr(), b.scans.data(), b.scans.size() * sizeof(JpegProgScan));
  if (!b.tabs.empty()) std::memcpy(pk->tabs.data_ptr(), b.tabs.data(), b.tabs.size() * sizeof(JpegHuffTab));
  static_assert(sizeof(JpegRstItem) == 4 * sizeof(int32_t), "an item is a row of four int32");
  pk->rst_items = torch::empty({(int64_t)b.rst_items.size(), 4}, torch::kInt32);
  if (!b.rst_items.empty())
    std::memcpy(pk->rst_items.data_ptr(), b.rst_items.data(), b.rst_items.size() * sizeof(JpegRstItem));
  std::vector<int32_t> prog_list;
  {
    py::gil_scoped_release nogil;
    if (b.byte_total) jpeg_huff_copy_bytes(b, ptr.data(), len.data(), pk->bytes.data_ptr<uint8_t>());
    if (!b.sets.empty()) std::memcpy(pk->sets.data_ptr(), b.sets.data(), b.sets.size() * sizeof(JpegHuffSet));
    if (!b.desc.empty()) std::memcpy(pk->desc.data_ptr(), b.desc.data(), b.desc.size() * sizeof(JpegHuffDesc));
  }
  pk->status.assign(status.begin(), status.end());
  pk->offs.assign(n, -1);
  for (int i = 0; i < n; ++i)
    if (b.desc[i].gpu) {
      pk->offs[i] = b.desc[i].coef_base;
      ++pk->n_gpu;
      if (b.desc[i].gpu == 3) prog_list.push_back(i);
      else if (b.desc[i].gpu == 4) ++pk->n_rst;
      else ++(b.desc[i].gpu == 2 ? pk->n_par : pk->n_lane);
    }
  pk->n_prog = (int64_t)prog_list.size();
  pk->prog_list = torch::empty({pk->n_prog}, torch::kInt32);
  if (pk->n_prog) std::memcpy(pk->prog_list.data_ptr(), prog_list.data(), prog_list.size() * sizeof(int32_t));
  pk->nsets = (int64_t)b.sets.size();
  pk->byte_total = b.byte_total;
  pk->coef_total = b.coef_total;
  return pk;
}

// The operand checks the two entropy launches share: bytes uint8 (the packed bytes, on the
// device), coefs int16 [>= coef_total], status int32 [n], and the packed batch unchanged.
static void check_entropy_operands(const char* op, const std::shared_ptr<JpegHuffPacked>& pk, const torch::Tensor& bytes,
                                   const torch::Tensor& coefs, const torch::Tensor& status) {
  check_operand(bytes, "bytes", torch::kUInt8, -1, bytes.device());
  check_operand(coefs, "coefs", torch::kInt16, -1, bytes.device());
  check_operand(status, "status", torch::kInt32, -1, bytes.device());
  TORCH_CHECK(status.numel() >= pk->n && pk->n < (1ll << 31), op, ": status buffer too small");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(bytes.data_ptr()) % 16 == 0, op, ": bytes must be 16-byte aligned");
  TORCH_CHECK(pk->desc.numel() == pk->n * (int64_t)sizeof(JpegHuffDesc) &&
                  pk->sets.numel() == pk->nsets * (int64_t)sizeof(JpegHuffSet) &&
                  pk->scans.numel() == pk->nscans * (int64_t)sizeof(JpegProgScan) &&
                  pk->tabs.numel() == pk->ntabs * (int64_t)sizeof(JpegHuffTab) && pk->prog_list.numel() == pk->n_prog &&
                  pk->ntabs < (1ll << 31) && pk->rst_items.dim() == 2 && pk->rst_items.size(1) == 4 &&
                  pk->rst_items.is_contiguous() && pk->rst_items.scalar_type() == torch::kInt32 &&
                  (pk->n_rst > 0) == (pk->rst_items.size(0) > 0), op, ": packed batch changed");
}

// The progressive entries of a packed batch (gpu == 3), one lane each, into the same coefs / status on
// the current stream; the caller has run jpeg_huff_check / jpeg_huff_par_check with pk->opt.
static void launch_progressive(const char* op, const std::shared_ptr<JpegHuffPacked>& pk, const torch::Tensor& bytes,
                               const torch::Tensor& dev_desc, torch::Tensor& coefs, torch::Tensor& status) {
  if (pk->n_prog == 0) return;
  const char* why = jpeg_huff_prog_check(reinterpret_cast<const JpegHuffDesc*>(pk->desc.data_ptr()), (int)pk->n,
                                         reinterpret_cast<const JpegProgScan*>(pk->scans.data_ptr()), pk->nscans,
                                         pk->ntabs);
  TORCH_CHECK(why == nullptr, op, ": progressive descriptor outside its buffer: ", why ? why : "");
  const int32_t* lp = pk->prog_list.data_ptr<int32_t>();
  const auto* hd = reinterpret_cast<const JpegHuffDesc*>(pk->desc.data_ptr());
  for (int64_t j = 0; j < pk->n_prog; ++j)
    TORCH_CHECK(lp[j] >= 0 && lp[j] < pk->n && hd[lp[j]].gpu == 3, op, ": packed batch changed");
  auto dev_scans = pk->scans.to(bytes.device());
  auto dev_tabs = pk->tabs.to(bytes.device());
  auto dev_list = pk->prog_list.to(bytes.device());
  jpeg_entropy_prog_launch(bytes.data_ptr<uint8_t>(), reinterpret_cast<const JpegHuffTab*>(dev_tabs.data_ptr()),
                           (int)pk->ntabs, reinterpret_cast<const JpegProgScan*>(dev_scans.data_ptr()), pk->nscans,
                           reinterpret_cast<const JpegHuffDesc*>(dev_desc.data_ptr()), (int)pk->n,
                           dev_list.data_ptr<int32_t>(), (int)pk->n_prog, coefs.data_ptr<int16_t>(),
                           status.data_ptr<int>(), cur_stream());
  check_launch("jpeg_entropy_prog");
}

// The restart-interval entries of a packed batch (gpu == 4), one lane per interval, into the same coefs /
// status on the current stream; the caller has run jpeg_huff_check / jpeg_huff_par_check with pk->opt.
// The kernel only raises the status of an entry one of whose intervals is refused (atomic max) and writes
// nothing for an accepted one, so status must be zero on entry: runtime/jpeg.py _entropy_on_device
// allocates it with torch.zeros, and no other kernel writes the status of a gpu == 4 entry.
static void launch_restart(const char* op, const std::shared_ptr<JpegHuffPacked>& pk, const torch::Tensor& bytes,
                           const torch::Tensor& dev_desc, const torch::Tensor& dev_sets, torch::Tensor& coefs,
                           torch::Tensor& status) {
  if (pk->n_rst == 0) return;
  const char* why = jpeg_huff_rst_check(reinterpret_cast<const JpegHuffDesc*>(pk->desc.data_ptr()), (int)pk->n,
                                        reinterpret_cast<const JpegRstItem*>(pk->rst_items.data_ptr()),
                                        pk->rst_items.size(0));
  TORCH_CHECK(why == nullptr, op, ": restart-interval item outside its entry: ", why ? why : "");
  auto dev_items = pk->rst_items.to(bytes.device());
  jpeg_entropy_rst_launch(bytes.data_ptr<uint8_t>(), reinterpret_cast<const JpegHuffSet*>(dev_sets.data_ptr()),
                          reinterpret_cast<const JpegHuffDesc*>(dev_desc.data_ptr()),
                          reinterpret_cast<const JpegRstItem*>(dev_items.data_ptr()), (int)pk->rst_items.size(0),
                          coefs.data_ptr<int16_t>(), status.data_ptr<int>(), (int)pk->n, cur_stream());
  check_launch("jpeg_entropy_rst");
}

// Both entropy entry points: operand checks, every descriptor against these very buffers, descriptor
// uploads, then the one-lane kernel, the sub-stream kernel (scratch != nullptr: a batch packed with
// parallel = true), the interval kernel and the progressive kernel, each on its own entries, all into
// the same coefs / status on the current stream.
static void entropy_launch(const char* op, const std::shared_ptr<JpegHuffPacked>& pk, torch::Tensor& bytes,
                           torch::Tensor& coefs, torch::Tensor& status, torch::Tensor* scratch) {
  if (pk->n_gpu == 0) return;
  check_entropy_operands(op, pk, bytes, coefs, status);
  const auto* hd = reinterpret_cast<const JpegHuffDesc*>(pk->desc.data_ptr());
  const char* why;
  if (scratch != nullptr) {
    check_operand(*scratch, "scratch", torch::kInt32, -1, bytes.device());
    TORCH_CHECK(pk->par.numel() == pk->n * (int64_t)sizeof(JpegParDesc), op, ": packed batch changed");
    why = jpeg_huff_par_check(hd, reinterpret_cast<const JpegParDesc*>(pk->par.data_ptr()), (int)pk->n, bytes.numel(),
                              pk->nsets, coefs.numel(), scratch->numel(), kJpegParSubBits, pk->opt);
  } else {
    why = jpeg_huff_check(hd, (int)pk->n, bytes.numel(), pk->nsets, coefs.numel(), pk->opt);
  }
  TORCH_CHECK(why == nullptr, op, ": descriptor outside its buffer: ", why ? why : "");
  auto dev_desc = pk->desc.to(bytes.device());
  auto dev_sets = pk->sets.to(bytes.device());
  torch::Tensor dev_par;                     // every upload before the first launch: none waits for a kernel
  if (scratch != nullptr) dev_par = pk->par.to(bytes.device());
  const auto* sp = reinterpret_cast<const JpegHuffSet*>(dev_sets.data_ptr());
  const auto* dp = reinterpret_cast<const JpegHuffDesc*>(dev_desc.data_ptr());
  if (pk->n_lane) {
    jpeg_entropy_launch(bytes.data_ptr<uint8_t>(), sp, dp, coefs.data_ptr<int16_t>(), status.data_ptr<int>(),
                        (int)pk->n, cur_stream());
    check_launch("jpeg_entropy");
  }
  if (scratch != nullptr && pk->n_par) {
    jpeg_entropy_par_launch(bytes.data_ptr<uint8_t>(), sp, dp, reinterpret_cast<const JpegParDesc*>(dev_par.data_ptr()),
                            coefs.data_ptr<int16_t>(), status.data_ptr<int>(),
                            reinterpret_cast<uint32_t*>(scratch->data_ptr<int>()), (int)pk->n, cur_stream());
    check_launch("jpeg_entropy_par");
  }
  launch_restart(op, pk, bytes, dev_desc, dev_sets, coefs, status);
  launch_progressive(op, pk, bytes, dev_desc, coefs, status);
}

// Decodes the packed batch into coefs (zeroed by the caller: jpeg_entropy_zero) on the current
// stream; status is written for the accepted entries only (zero on entry: see launch_restart).
void jpeg_entropy_gpu(const std::shared_ptr<JpegHuffPacked>& pk, torch::Tensor bytes, torch::Tensor coefs,
                      torch::Tensor status) {
  TORCH_CHECK(pk != nullptr, "no packed batch");
  TORCH_CHECK(!pk->parallel, "jpeg_entropy_gpu: the batch was packed for jpeg_entropy_gpu_parallel");
  entropy_launch("jpeg_entropy_gpu", pk, bytes, coefs, status, nullptr);
}

// The same for a batch packed with parallel = true: the sub-stream kernel on the entries laid out
// for it, the one-lane kernel on the rest (restart markers), both into the same coefs / status.
// scratch int32 [>= scratch_total]: the sub-stream state of the images too long for LDS.
void jpeg_entropy_gpu_parallel(const std::shared_ptr<JpegHuffPacked>& pk, torch::Tensor bytes, torch::Tensor coefs,
                               torch::Tensor status, torch::Tensor scratch) {
  TORCH_CHECK(pk != nullptr, "no packed batch");
  TORCH_CHECK(pk->parallel, "jpeg_entropy_gpu_parallel: the batch was packed for jpeg_entropy_gpu");
  entropy_launch("jpeg_entropy_gpu_parallel", pk, bytes, coefs, status, &scratch);
}

// Measurement helper (tools/jpeg_bench.py): the synchronisation rounds the sub-stream kernel needs for
// each entry, found by running the rounds of jpeg_huff_par.h on the host with one virtual thread at the
// kernel's sub-stream size and cap.  -1: not an entry that kernel takes; 0: not converged within the cap.
std::vector<int64_t> jpeg_huff_par_rounds(py::list datas) {
  const int n = (int)datas.size();
  std::vector<const uint8_t*> ptr;
  std::vector<size_t> len;
  bytes_list(datas, &ptr, &len);
  std::vector<int64_t> rounds(n, -1);
  py::gil_scoped_release nogil;
  std::vector<JpegHeader> hdr((size_t)n);
  std::vector<int> status(n, JPEG_EMPTY);
  JpegHuffBatch b;
  jpeg_huff_plan(n, ptr.data(), len.data(), hdr.data(), status.data(), &b, kJpegParSubBits);
  std::vector<uint8_t> bytes((size_t)b.byte_total + 4);
  jpeg_huff_copy_bytes(b, ptr.data(), len.data(), bytes.data());
  std::vector<uint32_t> words(bytes.size() / 4);
  std::memcpy(words.data(), bytes.data(), words.size() * 4);
  std::vector<uint32_t> st;
  for (int i = 0; i < n; ++i) {
    const JpegHuffDesc& d = b.desc[(size_t)i];
    if (d.gpu != 2) continue;
    const JpegParDesc& p = b.par[(size_t)i];
    const uint32_t nsub = jpeg_par_nsub(p.bit_len, kJpegParSubBits);
    st.assign((size_t)kJpegParStateWords * nsub, 0u);
    const JpegParCtx x{&d, &p, words.data() + d.byte_off / 4, &b.sets[(size_t)d.set_idx], st.data(), nullptr,
                       kJpegParSubBits, nsub};
    jpeg_par_init(x, 0, 1);
    const uint32_t R = nsub < kJpegParMaxRounds ? nsub : kJpegParMaxRounds;
    int cur = 0;
    rounds[i] = 0;
    for (uint32_t r = 0; r < R; ++r) {
      if (!jpeg_par_round(x, cur, 0, 1)) {
        rounds[i] = (int64_t)r + 1;
        break;
      }
      cur ^= 1;
    }
  }
  return rounds;
}

void jpeg_entropy_zero(torch::Tensor coefs) {
  check_operand(coefs, "coefs", torch::kInt16, -1, coefs.device());
  jpeg_entropy_zero_launch(coefs.data_ptr<int16_t>(), coefs.numel(), cur_stream());
  check_launch("jpeg_entropy_zero");
}

// JpegPlan and JpegHuffPacked are complete types only here, so this family registers itself.
void bind_jpeg(py::module_& m) {
  m.def("jpeg_parse", &jpeg_parse, "JPEG markers up to SOS (native_progressive: of a progressive file up to EOI): "
        "(status, reason, header dict or None)", py::arg("data"), py::arg("native_progressive") = false,
        py::arg("native_sampling") = false, py::arg("native_colorspace") = false);
  m.def("jpeg_entropy_batch", &jpeg_entropy_batch,
        "baseline JPEG entropy decode of a list of bytes / None on native threads (GIL released): "
        "(status, headers, int16 coefficients on the host, offsets)", py::arg("datas"), py::arg("threads") = 8,
        py::arg("native_progressive") = false, py::arg("native_sampling") = false, py::arg("native_colorspace") = false);
  py::class_<JpegPlan, std::shared_ptr<JpegPlan>>(m, "JpegPlan")
      .def_readonly("n_gpu", &JpegPlan::n_gpu)
      .def_readonly("n_exact", &JpegPlan::n_exact)
      .def_readonly("n_color", &JpegPlan::n_color)
      .def_readonly("nblocks", &JpegPlan::nblocks)
      .def_readonly("coef_elems", &JpegPlan::coef_elems)
      .def_readonly("plane_bytes", &JpegPlan::plane_bytes)
      .def_readonly("out_bytes", &JpegPlan::out_bytes)
      .def_readonly("max_pix", &JpegPlan::max_pix)
      .def_readonly("out_off", &JpegPlan::out_off)
      .def_readonly("full_res", &JpegPlan::full_res);
  m.def("jpeg_plan", &jpeg_plan, "validate a decoded batch and build its device descriptor tables",
        py::arg("hdr"), py::arg("status"), py::arg("offs"), py::arg("coef_elems"), py::arg("geom"), py::arg("crop"),
        py::arg("device"));
  py::class_<JpegHuffPacked, std::shared_ptr<JpegHuffPacked>>(m, "JpegHuffPacked")
      .def_readonly("status", &JpegHuffPacked::status)
      .def_readonly("offs", &JpegHuffPacked::offs)
      .def_readonly("hdr", &JpegHuffPacked::hdr)
      .def_readonly("bytes", &JpegHuffPacked::bytes)
      .def_readonly("n", &JpegHuffPacked::n)
      .def_readonly("n_gpu", &JpegHuffPacked::n_gpu)
      .def_readonly("nsets", &JpegHuffPacked::nsets)
      .def_readonly("byte_total", &JpegHuffPacked::byte_total)
      .def_readonly("coef_total", &JpegHuffPacked::coef_total)
      .def_readonly("parallel", &JpegHuffPacked::parallel)
      .def_readonly("n_par", &JpegHuffPacked::n_par)
      .def_readonly("n_lane", &JpegHuffPacked::n_lane)
      .def_readonly("scratch_total", &JpegHuffPacked::scratch_total)
      .def_property_readonly("native_progressive", [](const JpegHuffPacked& p) { return p.opt.native_progressive; })
      .def_readonly("n_prog", &JpegHuffPacked::n_prog)
      .def_readonly("nscans", &JpegHuffPacked::nscans)
      .def_readonly("ntabs", &JpegHuffPacked::ntabs)
      .def_property_readonly("restart_intervals", [](const JpegHuffPacked& p) { return p.opt.restart_intervals; })
      .def_readonly("rst_items", &JpegHuffPacked::rst_items)
      .def_readonly("n_rst", &JpegHuffPacked::n_rst)
      .def_property_readonly("native_sampling", [](const JpegHuffPacked& p) { return p.opt.native_sampling; })
      .def_property_readonly("native_colorspace", [](const JpegHuffPacked& p) { return p.opt.native_colorspace; });
  m.def("jpeg_huff_pack", &jpeg_huff_pack,
        "parse a list of bytes / None and pack bytes, Huffman tables and descriptors for the device entropy stage "
        "(parallel: the sub-stream layout of jpeg_entropy_gpu_parallel; the other flags: JpegOptions)",
        py::arg("datas"), py::arg("parallel") = false, py::arg("native_progressive") = false,
        py::arg("restart_intervals") = false, py::arg("native_sampling") = false, py::arg("native_colorspace") = false);
  m.attr("JPEG_PROG_MAX_SCANS") = (int64_t)kJpegProgMaxScans;
  m.attr("JPEG_HEADER_PROGRESSIVE_OFFSET") = (int64_t)offsetof(JpegHeader, progressive);   // an int, in the header rows
  m.attr("JPEG_HEADER_MODE_OFFSET") = (int64_t)offsetof(JpegHeader, mode);                 // likewise
  m.attr("JPEG_HEADER_COLORSPACE_OFFSET") = (int64_t)offsetof(JpegHeader, colorspace);     // likewise
  m.attr("JPEG_PAR_SUB_BITS") = (int64_t)kJpegParSubBits;
  m.attr("JPEG_PAR_THREADS") = (int64_t)kJpegParThreads;
  m.attr("JPEG_PAR_MAX_ROUNDS") = (int64_t)kJpegParMaxRounds;
  m.def("jpeg_entropy_zero", &jpeg_entropy_zero, "async memset of a device coefficient buffer", py::arg("coefs"));
  m.def("jpeg_entropy_gpu", &jpeg_entropy_gpu,
        "Huffman-decode a packed batch on the device: one lane per image, int32 status per image",
        py::arg("packed"), py::arg("bytes"), py::arg("coefs"), py::arg("status"));
  m.def("jpeg_entropy_gpu_parallel", &jpeg_entropy_gpu_parallel,
        "Huffman-decode a batch packed with parallel=True: one workgroup per image on self-synchronising "
        "sub-streams, restart-marker files on the one-lane kernel; status 100: not synchronised",
        py::arg("packed"), py::arg("bytes"), py::arg("coefs"), py::arg("status"), py::arg("scratch"));
  m.def("jpeg_huff_par_rounds", &jpeg_huff_par_rounds,
        "synchronisation rounds the sub-stream kernel needs per entry, emulated on the host (-1: not its entry, "
        "0: not within the cap)", py::arg("datas"));
  m.def("jpeg_idct", &jpeg_idct, "dequantise + 8x8 IDCT of a planned batch into uint8 component planes",
        py::arg("plan"), py::arg("coefs"), py::arg("planes"));
  m.def("jpeg_resize_crop", &jpeg_resize_crop,
        "component planes -> RGB uint8, chroma upsampled, resized and cropped as libjpeg + Pillow do",
        py::arg("plan"), py::arg("planes"), py::arg("out"));
}
