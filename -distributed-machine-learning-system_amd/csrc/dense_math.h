// Band planner of the fused DenseNet layer (kernels/dense.hip): pure host arithmetic, shared by the
// launcher, the binding's shape predicate and the host-side unit check (ops.dense_plan).
//
// LDS of a dense-layer workgroup, in this order:
//   x chunk   16 mf rows of kcb + 16 bytes: the K chunk of the 1x1's B operand (kcb = 64 .. 512 bytes of
//             channels, a multiple of the 64-byte MFMA K step, so a row is an odd number of 16-byte slots)
//   norm1     2 cin floats: scale then shift, read by the staging pass
//   map       (R + 2) x (W + 2) bottleneck pixels of 128 sizeof(T) + 16 bytes (17 or 33 slots)
#pragma once

namespace idunno {
namespace dense {

constexpr int kM = 128;           // bottleneck width
constexpr int kG = 32;            // growth: channels a layer appends
constexpr int kMaxW = 64;         // widest image planned for (a 56-wide fp32 band is then >= 2 rows)
constexpr int kMaxCin = 4096;
constexpr int kStepBytes = 64;    // one MFMA K step of either precision: 32 halfs or 16 floats
constexpr int kMaxChunkBytes = 512;
constexpr int kSmallBudget = 80 * 1024, kBudget = 160 * 1024;

struct Plan {
  int R, nbands;     // band height, bands an image
  int mf;            // pixel chunk of the 1x1: 16 mf pixels
  int kc;            // K chunk in elements
  int xbytes;        // x chunk region
  int ssbytes;       // norm1 region
  int lds;           // all of it
};

constexpr int map_pitch(int sz) { return kM * sz + 16; }

// largest K chunk (bytes) <= cap whose 64 rows fit in `room`; 0 when not even `floor` bytes fit
inline int chunk_bytes(int room, int cap, int floor_) {
  int kcb = (room / 64 - 16) / kStepBytes * kStepBytes;
  kcb = kcb < cap ? kcb : cap;
  return kcb >= floor_ ? kcb : 0;
}

inline bool plan_budget(int H, int W, int cin, int sz, int budget, bool whole_only, int min_chunk, Plan& p) {
  const int rowb = (W + 2) * map_pitch(sz), ss = 2 * cin * 4;
  const int cap = cin * sz < kMaxChunkBytes ? cin * sz : kMaxChunkBytes;
  const int floor_ = cap < min_chunk ? cap : min_chunk;
  int R = H;
  int kcb = chunk_bytes(budget - ss - (H + 2) * rowb, cap, floor_);   // the whole image as one band
  if (!kcb) {
    if (whole_only) return false;
    // several bands: the widest chunk that leaves a band at all, then the tallest band, balanced over the image
    for (kcb = cap; kcb >= floor_; kcb -= kStepBytes)
      if ((budget - ss - 64 * (kcb + 16)) / rowb - 2 >= 1) break;
    if (kcb < floor_) return false;
    int rmax = (budget - ss - 64 * (kcb + 16)) / rowb - 2;
    rmax = rmax < H ? rmax : H;
    const int nb = (H + rmax - 1) / rmax;
    R = (H + nb - 1) / nb;
  }
  int mf = 4;
  const int rows = (R + 2 < H ? R + 2 : H) * W;     // most pixels a band's 1x1 walks
  while (mf > 1 && 16 * (mf / 2) >= rows) mf /= 2;
  p.R = R;
  p.nbands = (H + R - 1) / R;
  p.mf = mf;
  p.kc = kcb / sz;
  p.xbytes = 16 * mf * (kcb + 16);
  p.ssbytes = ss;
  p.lds = p.xbytes + ss + (R + 2) * rowb;
  return p.lds <= budget;
}

// 80 KiB (two workgroups a CU) where the whole image is one band with K chunks of >= 256 bytes, else up to
// 160 KiB with chunks of >= 128
inline bool plan(int H, int W, int cin, bool f32, Plan& p) {
  if (H <= 0 || W <= 0 || W > kMaxW || cin <= 0 || cin % 32 || cin > kMaxCin) return false;
  const int sz = f32 ? 4 : 2;
  return plan_budget(H, W, cin, sz, kSmallBudget, true, 256, p) ||
         plan_budget(H, W, cin, sz, kBudget, false, 128, p);
}

}  // namespace dense
}  // namespace idunno
