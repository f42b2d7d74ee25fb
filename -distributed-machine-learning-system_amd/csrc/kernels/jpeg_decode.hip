// JPEG decode on the GPU, after the host's entropy decode (runtime/jpeg_entropy.cpp):
//
//   * jpeg_idct_kernel         int16 coefficients (not dequantised, natural order)
//                              -> uint8 component planes.  One wave = 8 blocks x 8
//                              rows: lane (b, r) loads row r of block b (16 bytes;
//                              a wave reads 1 KiB contiguous), dequantises and runs
//                              the row pass in registers, the tile is transposed in
//                              LDS (block stride 72 floats: the 8 blocks of a wave
//                              fall on disjoint banks for the column reads), lane
//                              (b, x) runs the column pass, +128, round half up,
//                              clamp, and a second LDS transpose of the bytes puts
//                              row y of two horizontally adjacent blocks side by
//                              side: the pair's even lane stores 16 bytes (plane
//                              pitch rounded up to 16).
//   * jpeg_idct_exact_kernel   the planes of mode-3 / mode-4 images (4:4:0, 4:1:1) again
//                              in fp64 over the former's output, so that their
//                              samples round as the float64 model's; launched only
//                              for a batch that holds such an image.  The planes of
//                              RGB / CMYK / YCCK images (colorspace != 0) as well.
//   * jpeg_resize_crop_kernel  one thread per output pixel: chroma "fancy"
//                              upsampling (libjpeg's integer triangle filters for
//                              h2v1, h2v2 and h1v2; replication for h4v1, as
//                              libjpeg has no filter for that ratio),
//                              YCbCr -> RGB rounded to uint8, Pillow's BILINEAR
//                              horizontal pass rounded to uint8, vertical pass
//                              rounded to uint8, centre crop.  rw == W / rh == H
//                              makes a pass the identity (full-resolution mode).
//                              A second instantiation, launched for a batch that
//                              holds an image with colorspace != 0, adds the colour
//                              stages of RGB-coded files (the planes as they are,
//                              planes 1 and 2 upsampled like chroma), CMYK and YCCK
//                              (Pillow's integer CMYK -> RGB).
//
// Both index a per-image descriptor table (kernels.h JpegImageDesc) whose offsets
// and extents the host validated.  Plain C++ and vector stores only.
#include "../kernels.h"

namespace idunno {

namespace {

// cos(k pi / 16)
__device__ constexpr float cos16(int k) {
  constexpr float c[9] = {1.f,          0.98078528f, 0.92387953f, 0.83146961f, 0.70710678f,
                          0.55557023f,  0.38268343f, 0.19509032f, 0.f};
  k %= 32;
  if (k > 16) k = 32 - k;
  return k <= 8 ? c[k] : -c[16 - k];
}
// type-III DCT matrix: sample x from frequency u
__device__ constexpr float idct_m(int x, int u) { return (u == 0 ? 0.35355339f : 0.5f * cos16((2 * x + 1) * u)); }

constexpr int kTileStride = 72;   // floats per block tile: 64 + 8, a multiple of 4 (16-byte rows)

__device__ __forceinline__ int find_seg(const JpegSeg* __restrict__ segs, int nseg, int pair) {
  int lo = 0, hi = nseg - 1;               // largest s with segs[s].pair_start <= pair
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].pair_start <= pair) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

}  // namespace

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                        const JpegImageDesc* __restrict__ desc,
                                                        const JpegSeg* __restrict__ segs, int nseg, int nslots) {
  __shared__ __attribute__((aligned(16))) float tile[4][8 * kTileStride];
  __shared__ __attribute__((aligned(16))) uint8_t bytes[4][4][8][16];   // [wave][pair][row][two blocks' 8 pixels]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = lane >> 3, r = lane & 7;
  // slot = 2 * pair + half: blocks (2k, 2k + 1) of one block row sit in lanes b, b + 1 (b even)
  const int slot = (blockIdx.x * 4 + wave) * 8 + b;
  const bool inrange = slot < nslots;       // nslots is even: a pair is in range as a whole
  int img = 0, comp = 0, by = 0, bx = 0;
  float f[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) f[u] = 0.f;
  if (inrange) {
    const int pair = slot >> 1;
    const JpegSeg sg = segs[find_seg(segs, nseg, pair)];
    img = sg.img;
    comp = sg.comp;
    const int bw = desc[img].bw[comp], bwp = (bw + 1) >> 1;
    const int lp = pair - sg.pair_start;
    by = lp / bwp;
    bx = 2 * (lp - by * bwp) + (slot & 1);
    if (bx < bw) {                          // else: the block past an odd row's end, zeros into the padding
      const size_t cblk = (size_t)desc[img].blk_off[comp] + (size_t)by * bw + bx;
      const vec16 cv = *reinterpret_cast<const vec16*>(coef + cblk * 64 + r * 8);
      const vec16 qv = *reinterpret_cast<const vec16*>(&desc[img].q[comp][r * 8]);
      const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[2 * i] = (float)((int)(int16_t)(cw[i] & 0xFFFFu) * (int)(qw[i] & 0xFFFFu));
        f[2 * i + 1] = (float)((int)(int16_t)(cw[i] >> 16) * (int)(qw[i] >> 16));
      }
    }
  }
  // row pass: t[x] = sum_u M(x, u) f[u]   (this lane: vertical frequency r)
  float t[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) a = fmaf(idct_m(x, u), f[u], a);
    t[x] = a;
  }
  float* tb = &tile[wave][b * kTileStride];
  *reinterpret_cast<float4v*>(tb + r * 8) = float4v{t[0], t[1], t[2], t[3]};
  *reinterpret_cast<float4v*>(tb + r * 8 + 4) = float4v{t[4], t[5], t[6], t[7]};
  __syncthreads();
  // column pass: this lane is column x = r; o[y] = sum_v M(y, v) tile[v][x]
  float c[8];
#pragma unroll
  for (int v = 0; v < 8; ++v) c[v] = tb[v * 8 + r];
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    float a = 128.5f;                          // + 128, round half up by the floor below
#pragma unroll
    for (int v = 0; v < 8; ++v) a = fmaf(idct_m(y, v), c[v], a);
    a = fminf(fmaxf(floorf(a), 0.f), 255.f);
    bytes[wave][b >> 1][y][(b & 1) * 8 + r] = (uint8_t)a;
  }
  __syncthreads();
  // the even lane of a pair stores row r of both blocks: 16 bytes at a 16-byte-aligned address
  // (plane_off and pitch are multiples of 16, bx is even); bx * 8 + 16 <= pitch = 16 * ceil(bw / 2)
  if (inrange && (b & 1) == 0) {
    const JpegImageDesc& d = desc[img];
    const vec16 row = *reinterpret_cast<const vec16*>(&bytes[wave][b >> 1][r][0]);
    uint8_t* dst = planes + d.plane_off[comp] + (size_t)(by * 8 + r) * (size_t)d.pitch[comp] + bx * 8;
    *reinterpret_cast<vec16*>(dst) = row;
  }
}

namespace {

// the type-III DCT matrix [sample][frequency] in fp64: 0.5 cos((2x + 1) u pi / 16), column 0 times sqrt(1/2)
__constant__ double kIdctD[64] = {
    0.3535533905932738, 0.4903926402016152, 0.46193976625564337, 0.4157348061512726, 0.3535533905932738, 0.27778511650980114, 0.19134171618254492, 0.09754516100806417,
    0.3535533905932738, 0.4157348061512726, 0.19134171618254492, -0.0975451610080641, -0.35355339059327373, -0.4903926402016152, -0.4619397662556434, -0.2777851165098011,
    0.3535533905932738, 0.27778511650980114, -0.19134171618254486, -0.4903926402016152, -0.35355339059327384, 0.09754516100806415, 0.46193976625564326, 0.41573480615127273,
    0.3535533905932738, 0.09754516100806417, -0.46193976625564337, -0.2777851165098011, 0.3535533905932737, 0.41573480615127273, -0.19134171618254495, -0.4903926402016153,
    0.3535533905932738, -0.0975451610080641, -0.4619397662556434, 0.2777851165098009, 0.35355339059327384, -0.41573480615127256, -0.19134171618254528, 0.4903926402016152,
    0.3535533905932738, -0.277785116509801, -0.19134171618254517, 0.4903926402016152, -0.35355339059327334, -0.09754516100806401, 0.46193976625564337, -0.4157348061512725,
    0.3535533905932738, -0.4157348061512727, 0.191341716182545, 0.09754516100806439, -0.35355339059327356, 0.4903926402016153, -0.4619397662556432, 0.27778511650980076,
    0.3535533905932738, -0.4903926402016152, 0.46193976625564326, -0.41573480615127256, 0.3535533905932733, -0.27778511650980076, 0.19134171618254478, -0.09754516100806429};

}  // namespace

// The planes of the images of mode 3 and 4 and of every image with colorspace != 0 once more, in fp64, over
// jpeg_idct_kernel's output (same slots, launched after it when the batch holds such an image; every other
// image's slots return at once).  An RGB-coded image hands every plane on undiluted and CMYK / YCCK multiply
// two planes, so there one level of a plane at an fp32 rounding tie is up to two levels of output.  Modes 3, 4: their
// colour stage hands a chroma sample on undiluted (mode 4 replicates it, mode 3 filters along one axis
// only), and R = Y + 1.402 Cr, B = Y + 1.772 Cb turn one level of chroma into two of colour, so a sample
// whose exact value lies within fp32's reach of a rounding tie (164.5000034 was met) must round as the
// float64 model rounds it.  Lane (b, x): column x of block b; row pass over the 64 dequantised coefficients
// (exact integers in fp64), column pass, + 128, round half up, clamp, one byte per row.
__global__ __launch_bounds__(256) void jpeg_idct_exact_kernel(const int16_t* __restrict__ coef,
                                                              uint8_t* __restrict__ planes,
                                                              const JpegImageDesc* __restrict__ desc,
                                                              const JpegSeg* __restrict__ segs, int nseg, int nslots) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = lane >> 3, x = lane & 7;
  const int slot = (blockIdx.x * 4 + wave) * 8 + b;           // jpeg_idct_kernel's numbering
  if (slot >= nslots) return;
  const int pair = slot >> 1;
  const JpegSeg sg = segs[find_seg(segs, nseg, pair)];
  const JpegImageDesc& d = desc[sg.img];
  if (d.colorspace == 0 && (d.ncomp != 3 || d.mode < 3)) return;
  const int comp = sg.comp;
  const int bw = d.bw[comp], bwp = (bw + 1) >> 1;
  const int lp = pair - sg.pair_start;
  const int by = lp / bwp;
  const int bx = 2 * (lp - by * bwp) + (slot & 1);
  if (bx >= bw) return;                                       // the block past an odd row's end: padding
  const int16_t* cb = coef + ((size_t)d.blk_off[comp] + (size_t)by * bw + bx) * 64;
  double mx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) mx[u] = kIdctD[x * 8 + u];
  double s[8];                                                // s[v] = sum_u M(x, u) F[v][u]
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const vec16 cv = *reinterpret_cast<const vec16*>(cb + v * 8);
    const vec16 qv = *reinterpret_cast<const vec16*>(&d.q[comp][v * 8]);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a = fma(mx[2 * i], (double)((int)(int16_t)(cw[i] & 0xFFFFu) * (int)(qw[i] & 0xFFFFu)), a);
      a = fma(mx[2 * i + 1], (double)((int)(int16_t)(cw[i] >> 16) * (int)(qw[i] >> 16)), a);
    }
    s[v] = a;
  }
  // bx * 8 + x < 8 * bw <= pitch, by * 8 + y < 8 * bh: inside the plane jpeg_plan laid out
  uint8_t* dst = planes + d.plane_off[comp] + (size_t)(by * 8) * (size_t)d.pitch[comp] + bx * 8 + x;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    double a = 128.5;                                         // + 128, round half up by the floor below
#pragma unroll
    for (int v = 0; v < 8; ++v) a = fma(kIdctD[y * 8 + v], s[v], a);
    dst[(size_t)y * (size_t)d.pitch[comp]] = (uint8_t)fmin(fmax(floor(a), 0.0), 255.0);
  }
}

namespace {

struct Planes {
  const uint8_t* y;
  const uint8_t* cb;
  const uint8_t* cr;
  int py, pc;          // pitches
  int cw, ch;          // chroma plane's valid size
  int mode, ncomp;
  // the kColor instantiation only: the fourth plane (CMYK / YCCK, as large as the first) and JpegImageDesc::colorspace
  const uint8_t* k;
  int pk, cs;
};

// one upsampled chroma sample at luma position (x, y)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pitch, int cw, int ch, int mode, int x,
                                         int y) {
  if (mode == 0) return p[(size_t)y * pitch + x];
  if (mode == 3) {                                   // h1v2: libjpeg's vertical triangle filter, columns as they are
    const int j = y >> 1;
    const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    return (3 * p[(size_t)j * pitch + x] + p[(size_t)jf * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  if (mode == 4) return p[(size_t)y * pitch + (x >> 2)];   // h4v1: replication, libjpeg has no filter for 4:1
  const int i = x >> 1;
  if (mode == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    const int c = row[i];
    if (x & 1) return i == cw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
    return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
  const uint8_t* nr = p + (size_t)j * pitch;
  const uint8_t* fr = p + (size_t)jf * pitch;
  const int t = 3 * nr[i] + fr[i];
  if (x & 1) {
    if (i == cw - 1) return (4 * t + 7) >> 4;
    return (3 * t + 3 * nr[i + 1] + fr[i + 1] + 7) >> 4;
  }
  if (i == 0) return (4 * t + 8) >> 4;
  return (3 * t + 3 * nr[i - 1] + fr[i - 1] + 8) >> 4;
}

__device__ __forceinline__ double to_u8d(double v) { return fmin(fmax(floor(v + 0.5), 0.0), 255.0); }

// Pillow's MULDIV255: a * b / 255 rounded half up, for a, b in [0, 255]
__device__ __forceinline__ int muldiv255(int a, int b) {
  const int t = a * b + 128;
  return ((t >> 8) + t) >> 8;
}

// the decoded RGB pixel (x, y) of the full-size image, each channel a whole number in [0, 255]
// (fp64: the products have up to six decimals, and a tie must round as the float64 model's)
// kColor: the image may be RGB-coded (P.cs 1), CMYK (2) or YCCK (3); else P.cs and P.k are not read
template <bool kColor>
__device__ __forceinline__ void rgb_at(const Planes& P, int x, int y, double& r, double& g, double& b) {
  const double Y = (double)P.y[(size_t)y * P.py + x];
  if (P.ncomp == 1) {
    r = g = b = Y;
    return;
  }
  if (kColor && (P.cs == 1 || P.cs == 2)) {
    int p1, p2;
    if (P.cs == 1 && (P.mode == 1 || P.mode == 2) && P.cw <= 2) {
      // libjpeg filters a half-width plane only when it is more than two samples wide, else it replicates;
      // a YCbCr pixel dilutes the difference, an RGB plane is the pixel.  x >> 1 < cw, y >> 1 < ch.
      const size_t at = (size_t)(P.mode == 2 ? y >> 1 : y) * P.pc + (x >> 1);
      p1 = P.cb[at];
      p2 = P.cr[at];
    } else {
      p1 = chroma_at(P.cb, P.pc, P.cw, P.ch, P.mode, x, y);
      p2 = chroma_at(P.cr, P.pc, P.cw, P.ch, P.mode, x, y);
    }
    if (P.cs == 1) {                                   // RGB: the planes as they are
      r = Y;
      g = (double)p1;
      b = (double)p2;
      return;
    }
    // CMYK as Pillow reads it (inverted): C, M, Y = 255 - plane, 255 - K = plane 3
    const int p0 = P.y[(size_t)y * P.py + x], nk = P.k[(size_t)y * P.pk + x];
    r = (double)(nk - muldiv255(255 - p0, nk));
    g = (double)(nk - muldiv255(255 - p1, nk));
    b = (double)(nk - muldiv255(255 - p2, nk));
    return;
  }
  const double cb = (double)(chroma_at(P.cb, P.pc, P.cw, P.ch, P.mode, x, y) - 128);
  const double cr = (double)(chroma_at(P.cr, P.pc, P.cw, P.ch, P.mode, x, y) - 128);
  r = to_u8d(Y + 1.402 * cr);
  g = to_u8d(Y - 0.344136 * cb - 0.714136 * cr);
  b = to_u8d(Y + 1.772 * cb);
  if (kColor && P.cs == 3) {                           // YCCK: C, M, Y = the R', G', B' of planes 0..2
    const int nk = P.k[(size_t)y * P.pk + x];
    r = (double)(nk - muldiv255((int)r, nk));
    g = (double)(nk - muldiv255((int)g, nk));
    b = (double)(nk - muldiv255((int)b, nk));
  }
}

// Pillow's BILINEAR taps of output position o on an axis resized in -> out
struct Axis {
  int lo, hi;
  double centre, inv_fs;
  __device__ __forceinline__ Axis(int o, int in, int out) {
    const double scale = (double)in / (double)out;
    const double fs = scale > 1.0 ? scale : 1.0;
    centre = ((double)o + 0.5) * scale;
    inv_fs = 1.0 / fs;
    lo = max(0, (int)(centre - fs + 0.5));
    hi = min(in, (int)(centre + fs + 0.5));
  }
  __device__ __forceinline__ double weight(int x) const {
    const double w = 1.0 - fabs(((double)x - centre + 0.5) * inv_fs);
    return w > 0.0 ? w : 0.0;
  }
};

// row y of the horizontally resized image at column rx, rounded to uint8
template <bool kColor>
__device__ __forceinline__ void hpass_at(const Planes& P, const Axis& ax, bool ident, int rx, int y, double& r,
                                         double& g, double& b) {
  if (ident) {
    rgb_at<kColor>(P, rx, y, r, g, b);
    return;
  }
  double fr, fg, fb;
  double ar = 0.0, ag = 0.0, ab = 0.0, ws = 0.0;
  for (int x = ax.lo; x < ax.hi; ++x) {
    const double w = ax.weight(x);
    rgb_at<kColor>(P, x, y, fr, fg, fb);
    ar += w * fr;
    ag += w * fg;
    ab += w * fb;
    ws += w;
  }
  const double inv = 1.0 / ws;
  r = to_u8d(ar * inv);
  g = to_u8d(ag * inv);
  b = to_u8d(ab * inv);
}

}  // namespace

template <bool kColor>
__global__ __launch_bounds__(256) void jpeg_resize_crop_kernel(const uint8_t* __restrict__ planes,
                                                               const JpegImageDesc* __restrict__ desc,
                                                               uint8_t* __restrict__ out) {
  const JpegImageDesc& d = desc[blockIdx.y];
  const int npix = d.out_w * d.out_h;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int oy = i / d.out_w, ox = i - oy * d.out_w;
  const int rx = ox + d.left, ry = oy + d.top;       // position in the resized image
  double r = 0.0, g = 0.0, b = 0.0;                   // outside it: zero, as PIL's crop pads
  if (rx >= 0 && rx < d.rw && ry >= 0 && ry < d.rh) {
    Planes P;
    P.y = planes + d.plane_off[0];
    P.py = d.pitch[0];
    P.ncomp = d.ncomp;
    P.mode = d.mode;
    const bool multi = kColor ? d.ncomp >= 3 : d.ncomp == 3;
    const int cc = multi ? 1 : 0;
    P.cb = planes + d.plane_off[cc];
    P.cr = planes + d.plane_off[multi ? 2 : 0];
    P.cs = 0;
    P.k = P.y;
    P.pk = P.py;
    if (kColor) {
      P.cs = d.colorspace;
      if (d.ncomp == 4) {
        P.k = planes + d.plane_off[3];
        P.pk = d.pitch[3];
      }
    }
    P.pc = d.pitch[cc];
    P.cw = d.cw[cc];
    P.ch = d.ch[cc];
    const bool hid = d.rw == d.W, vid = d.rh == d.H;
    const Axis ax(rx, d.W, d.rw);
    if (vid) {
      hpass_at<kColor>(P, ax, hid, rx, ry, r, g, b);
    } else {
      const Axis ay(ry, d.H, d.rh);
      double ar = 0.0, ag = 0.0, ab = 0.0, ws = 0.0;
      for (int y = ay.lo; y < ay.hi; ++y) {
        const double w = ay.weight(y);
        double hr, hg, hb;
        hpass_at<kColor>(P, ax, hid, rx, y, hr, hg, hb);
        ar += w * hr;
        ag += w * hg;
        ab += w * hb;
        ws += w;
      }
      const double inv = 1.0 / ws;
      r = to_u8d(ar * inv);
      g = to_u8d(ag * inv);
      b = to_u8d(ab * inv);
    }
  }
  uint8_t* o = out + d.out_off + (size_t)i * 3;
  o[0] = (uint8_t)r;
  o[1] = (uint8_t)g;
  o[2] = (uint8_t)b;
}

void jpeg_idct_launch(const int16_t* coef, uint8_t* planes, const JpegImageDesc* desc, const JpegSeg* segs, int nseg,
                      int nslots, hipStream_t st) {
  if (nslots <= 0) return;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nslots + 31) / 32)), dim3(256), 0, st, coef, planes, desc,
                     segs, nseg, nslots);
}

void jpeg_idct_exact_launch(const int16_t* coef, uint8_t* planes, const JpegImageDesc* desc, const JpegSeg* segs,
                            int nseg, int nslots, hipStream_t st) {
  if (nslots <= 0) return;
  hipLaunchKernelGGL(jpeg_idct_exact_kernel, dim3((unsigned)((nslots + 31) / 32)), dim3(256), 0, st, coef, planes,
                     desc, segs, nseg, nslots);
}

void jpeg_resize_crop_launch(const uint8_t* planes, const JpegImageDesc* desc, uint8_t* out, int nimg, int max_pix,
                             bool color, hipStream_t st) {
  if (nimg <= 0 || max_pix <= 0) return;
  const dim3 grid((unsigned)((max_pix + 255) / 256), (unsigned)nimg);
  if (color) hipLaunchKernelGGL(jpeg_resize_crop_kernel<true>, grid, dim3(256), 0, st, planes, desc, out);
  else hipLaunchKernelGGL(jpeg_resize_crop_kernel<false>, grid, dim3(256), 0, st, planes, desc, out);
}

}  // namespace idunno
