// Planner and index math of the fused ShuffleNetV2 unit (kernels/shuffle_unit.hip): __host__ __device__ and free of
// the standard library, shared by the kernel, the launcher, the binding's shape checks and ops.shuffle_plan.
//
// Widths of a unit with logical output width c (h = c / 2) and logical input width cin, element size sz:
//   Cp    roundup(c, 8): channels a stored pixel has; Cpin likewise for the input (stride 1: cin == c)
//   KS    64 / sz: one MFMA K step (32 halfs or 16 floats)
//   hp    roundup(h, KS): the branch width as GEMM N, as the LDS map's channels and as pw2's K
//   k0    first input channel pw1 walks: stride 1 floor8(h) (so h = 58 needs no unaligned access: the rows of w1
//         for channels k0 .. h - 1 are zero), stride 2 zero (pw1 sees every channel)
//   Kx    roundup(Cpin - k0, KS): pw1's K, zero-filled past Cpin
// Pixels in LDS are hp sz + 16 (map, pw2's operand) or Kx sz + 16 (staged input, branch 1's operand) bytes: an odd
// number of 16-byte slots, so the 16 pixel lanes of a 16-byte LDS read fall on 16 different slots.
//
// LDS of a workgroup (a band of R output rows of `imgs` images), in this order:
//   region 0   the staged input rows (stride 1: R + 2, stride 2: 2 R + 1, clipped to the image); once pw1 and branch
//              1's depthwise have read them the same bytes hold pw2's operand and, behind it at o1_off, branch 1's
//              output (stride 2)
//   map        relu(pw1) with the depthwise conv's zero border: rows x (W + 2) pixels
//   a1         stride 2 only: the operand of branch 1's 1x1
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IDUNNO_SHUFFLE_HD __host__ __device__
#else
#define IDUNNO_SHUFFLE_HD
#endif

namespace idunno {
namespace shuffle {

constexpr int kBudget = 160 * 1024;
constexpr int kMinPix = 64;       // a GEMM's M should reach four 16-row fragments: below it a workgroup takes more images
constexpr int kMaxImgs = 8;
constexpr int kMaxW = 256, kMaxC = 4096;

struct Plan {
  int R, nbands, imgs;            // output rows a band, bands an image, images a workgroup
  int Ho, Wo, cp, cpin;
  int k0, Kx, hp;
  int px, pm;                     // pixel pitches in bytes: staged input / map
  int o1_off, map_off, a1_off;    // region 0 starts at 0
  int lds;
};

IDUNNO_SHUFFLE_HD constexpr int rup(int v, int m) { return (v + m - 1) / m * m; }
IDUNNO_SHUFFLE_HD constexpr int out_size(int n, int stride) { return stride == 1 ? n : (n - 1) / 2 + 1; }
// input (and map) rows a band of R output rows needs
IDUNNO_SHUFFLE_HD constexpr int in_rows(int R, int stride) { return stride == 1 ? R + 2 : 2 * R + 1; }

IDUNNO_SHUFFLE_HD inline void dims(int cin, int c, int stride, int sz, Plan& p) {
  const int ks = 64 / sz, h = c / 2;
  p.cp = rup(c, 8);
  p.cpin = stride == 1 ? p.cp : rup(cin, 8);
  p.hp = rup(h, ks);
  p.k0 = stride == 1 ? h / 8 * 8 : 0;
  p.Kx = rup(p.cpin - p.k0, ks);
  p.px = p.Kx * sz + 16;
  p.pm = p.hp * sz + 16;
}

// fills the offsets for a band of R rows of `imgs` images; returns the LDS bytes
IDUNNO_SHUFFLE_HD inline int layout(int H, int W, int stride, int R, int imgs, Plan& p) {
  const int rin = in_rows(R, stride), rs = rin < H ? rin : H;
  const int xs = rup(imgs * rs * W, 16) * p.px;
  const int npo = rup(imgs * R * p.Wo, 16);
  p.o1_off = npo * p.pm;
  const int second = stride == 2 ? 2 * p.o1_off : p.o1_off;
  p.map_off = xs > second ? xs : second;
  p.a1_off = p.map_off + imgs * rin * (W + 2) * p.pm;
  p.lds = p.a1_off + (stride == 2 ? npo * p.px : 0);
  return p.lds;
}

// the tallest band that fits, balanced over the image; an image that fits is one band, and a small one shares its
// workgroup with others (stride 1 only: a stride-2 unit's staged input leaves no room)
IDUNNO_SHUFFLE_HD inline bool plan(int H, int W, int cin, int c, int stride, bool f32, Plan& p) {
  if (H <= 0 || W <= 0 || H > kMaxW || W > kMaxW || c <= 0 || c % 2 || c > kMaxC || cin <= 0 || cin > kMaxC) return false;
  if ((stride != 1 && stride != 2) || (stride == 1 && cin != c)) return false;
  dims(cin, c, stride, f32 ? 4 : 2, p);
  p.Ho = out_size(H, stride);
  p.Wo = out_size(W, stride);
  int R = p.Ho;
  while (R >= 1 && layout(H, W, stride, R, 1, p) > kBudget) --R;
  if (R < 1) return false;
  const int nb = (p.Ho + R - 1) / R;
  R = (p.Ho + nb - 1) / nb;
  int imgs = 1;
  if (stride == 1 && nb == 1)
    while (imgs * H * W < kMinPix && imgs < kMaxImgs && layout(H, W, stride, R, imgs + 1, p) <= kBudget) ++imgs;
  layout(H, W, stride, R, imgs, p);
  p.R = R;
  p.nbands = nb;
  p.imgs = imgs;
  return true;
}

// pixel m of a workgroup's pixel list (imgs images x rows x width) -> image, row, column
struct Pix {
  int img, r, c;
};
IDUNNO_SHUFFLE_HD inline Pix pix_of(int m, int rows, int width) {
  const int per = rows * width, img = m / per, rem = m - img * per, r = rem / width;
  return Pix{img, r, rem - r * width};
}

}  // namespace shuffle
}  // namespace idunno
