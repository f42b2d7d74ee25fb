// Baseline JPEG Huffman decode of ONE scan on many lanes, by self-synchronising
// sub-streams: the sibling of jpeg_huff_core.h (one lane per image), shared by the
// device kernel (kernels/jpeg_entropy.hip, jpeg_entropy_par_kernel: one workgroup
// per image) and the host (csrc/tests/jpeg_huff_par_checks.cpp, which runs the same
// phases with virtual threads against runtime/jpeg_entropy.cpp).
//
// The packer (runtime/jpeg_huff_pack.cpp) hands over the scan's bits with a plain
// index: FF 00 stuffing and fill bytes removed, cut at the first marker, stored as
// 32-bit words whose most significant byte comes first, so bit q of the stream is
// bit 31 - q % 32 of word q / 32.  Images with a restart interval do not come here.
//
// The bits are cut into sub-streams of S bits (a runtime argument, a multiple of
// 32).  Sub-stream j starts from a guessed state (bit j * S, zigzag index 0, block 0
// of the MCU).  Rounds: every lane decodes from its entry state to the first symbol
// boundary at or past (j + 1) * S, the exit becomes the entry of j + 1, a lane whose
// entry did not change does not decode again, and the rounds end when no entry
// changed.  The fixed point is the sequential decode's (lane 0 starts from the true
// state, and lane j is right one round after lane j - 1), so it is reached within
// as many rounds as there are sub-streams; in practice a wrong lane falls into step
// with the true symbol boundaries after a few dozen symbols.  For that a lane
// decoding from a wrong state never gives up: an unknown code consumes one bit, a
// zigzag index past 63 ends the block, a DC category above 15 is masked.  Errors
// count only in the write pass, whose entry states are the true ones up to the
// first error.
//
// Phases, each over the sub-streams t, t + T, ... of thread t, a barrier between
// them (the state lives in 6 words per sub-stream at JpegParCtx::st):
//   jpeg_par_init      every entry := the guess, flagged "changed"
//   jpeg_par_round     (repeated) flagged lanes decode leniently and record blocks
//                      completed + per-component DC sums; every lane hands its exit
//                      to the other entry buffer, flagged where it differs
//   jpeg_par_partial / jpeg_par_scan   exclusive prefix of blocks and DC sums: each
//                      lane's first block number in scan order and its predictors
//   jpeg_par_write     strict decode, every store checked as in jpeg_huff_core.h
#pragma once
#include "jpeg_huff_core.h"

namespace idunno {

constexpr int kJpegHuffUnsynced = 100;          // device-only: above every JpegStatus value
constexpr uint32_t kJpegParMaxBits = 1u << 30;  // longer scans keep the one-lane kernel
constexpr int kJpegParStateWords = 6;           // per sub-stream: entry x2, blocks, DC sum x3
constexpr uint32_t kJpegParChanged = 1u << 31;
constexpr uint32_t kJpegParMaxSubBits = 1u << 16;
// What the kernel runs with.  kJpegParMaxRounds is a safety cap, not a tuning knob:
// an image that has not converged by then is reported kJpegHuffUnsynced and decoded
// by the fallback.  The largest round count csrc/tests/jpeg_huff_par_checks.cpp
// prints over all its inputs (files, prefixes, mutants) at kJpegParSubBits is 30
// (4 x 30 = 120); a 640x480 4:4:4 noise image at quality 95 (5,797 sub-streams)
// takes 42, the 2,000 photograph-like files of tools/jpeg_bench.py 6 to 15.  The
// cap is 256.
constexpr uint32_t kJpegParSubBits = 1024;
constexpr uint32_t kJpegParThreads = 256;
constexpr uint32_t kJpegParMaxRounds = 256;

// One per batch entry next to its JpegHuffDesc; meaningful where JpegHuffDesc::gpu == 2.
// The descriptor's byte span then holds the de-stuffed words (byte_len = the
// de-stuffed bytes, byte_span = that rounded up to whole words).
struct JpegParDesc {
  int64_t scratch_off;     // first state word of this image in the batch scratch buffer (uint32 elements)
  uint32_t bit_len;        // 8 * byte_len, < kJpegParMaxBits
  uint32_t total_blocks;   // mcux * mcuy * bpm
  int32_t bpm;             // blocks per MCU: sum of h[c] * v[c]
  uint32_t scan_pos;       // host only: where the scan starts in the file (the packer's copy)
};

JH_HD inline uint32_t jpeg_par_nsub(uint32_t bit_len, uint32_t sub_bits) {
  const uint32_t n = bit_len / sub_bits + (bit_len % sub_bits ? 1u : 0u);
  return n ? n : 1u;
}

struct JpegParCtx {
  const JpegHuffDesc* d;
  const JpegParDesc* p;
  const uint32_t* words;   // d->byte_span / 4 words
  const JpegHuffSet* set;
  uint32_t* st;            // kJpegParStateWords * nsub words
  int16_t* coef;           // the image's own span, zeroed
  uint32_t sub_bits, nsub;
};

namespace jpeg_huff_detail {

// MSB-first reader at a plain bit index; past the last word it yields zero bits.
struct ParBits {
  const uint32_t* words;
  uint32_t nwords, pos, wi;
  uint64_t acc;

  JH_HD void init(const uint32_t* words_, uint32_t nwords_, uint32_t pos_) {
    words = words_;
    nwords = nwords_;
    pos = pos_;
    load();
  }
  JH_HD void load() {
    wi = pos >> 5;
    const uint32_t a = wi < nwords ? words[wi] : 0u;
    const uint32_t b = wi + 1u < nwords ? words[wi + 1u] : 0u;
    acc = ((uint64_t)a << 32) | b;
  }
  // k in 1..16: bits [pos, pos + k)
  JH_HD unsigned peek(int k) {
    if ((pos >> 5) != wi) load();
    return (unsigned)((acc << (pos & 31u)) >> (64 - k));
  }
  JH_HD void skip(int k) { pos += (uint32_t)k; }
};

JH_HD inline uint32_t par_pack(uint32_t rel, int k, int b) { return rel | ((uint32_t)k << 8) | ((uint32_t)b << 16); }

}  // namespace jpeg_huff_detail

// Decodes from (pos, k, b) up to the first symbol boundary at or past `limit`;
// pos / k / b leave as the exit state, nblk counts the blocks completed, dc[c]
// gains the DC differences met (wrapping: exact wherever the true predictors fit
// int16).  Lenient (!kStrict): touches no coefficient and never fails.  Strict:
// first_block is the scan-order number of the block the entry state is in and dc[]
// enters as the predictors; stores coefficients, stops once the scan's last block
// is done, and returns kJpegHuffCorrupt on what jpeg_decode refuses.
template <bool kStrict>
JH_HD inline int jpeg_par_lane(const JpegHuffDesc& d, const JpegParDesc& p, const uint32_t* words,
                               const JpegHuffSet& set, uint32_t limit, uint32_t& pos, int& k, int& b, uint32_t& nblk,
                               uint32_t dc[3], uint32_t first_block, int16_t* coef) {
  using namespace jpeg_huff_detail;
  ParBits br;
  br.init(words, d.byte_span / 4u, pos);
  const int n0 = d.h[0] * d.v[0];
  const int n1 = d.ncomp == 3 ? n0 + d.h[1] * d.v[1] : p.bpm;
  int c = b < n0 ? 0 : (b < n1 ? 1 : 2);
  long long base = -1;                          // strict: first element of the current block, -1: not placed yet
  nblk = 0;
  const uint32_t maxsym = pos < limit ? limit - pos : 0u;   // every symbol consumes at least one bit
  for (uint32_t it = 0; it < maxsym && br.pos < limit; ++it) {
    const int sym = symbol(br, k == 0 ? set.dc[d.td[c]] : set.ac[d.ta[c]]);
    if (sym < 0) {
      if (kStrict) return kJpegHuffCorrupt;
      br.skip(1);
      continue;
    }
    const int s = sym & 15;
    int val = 0;
    bool has = false;
    if (k == 0) {
      if (kStrict && sym > 15) return kJpegHuffCorrupt;
      if (s) dc[c] += (uint32_t)extend(br, s);
      val = (int)(int32_t)dc[c];
      if (kStrict && (val < -32768 || val > 32767)) return kJpegHuffCorrupt;
      has = true;
    } else {
      const int r = sym >> 4;
      if (s == 0) {
        if (r != 15) {
          k = 64;                               // EOB
        } else {
          k += 16;                              // ZRL
          if (kStrict && k > 64) return kJpegHuffCorrupt;
        }
      } else {
        k += r;
        if (k > 63) {
          if (kStrict) return kJpegHuffCorrupt;
        } else {
          val = extend(br, s);
          has = true;
        }
      }
    }
    if (has) {
      if (kStrict) {
        if (base < 0) {
          const uint32_t blk = first_block + nblk;          // < total_blocks: the lane stops there
          const uint32_t mcu = blk / (uint32_t)p.bpm;
          const int my = (int)(mcu / (uint32_t)d.mcux), mx = (int)(mcu % (uint32_t)d.mcux);
          const int bi = b - (c == 0 ? 0 : (c == 1 ? n0 : n1));
          const int gx = mx * d.h[c] + bi % d.h[c], gy = my * d.v[c] + bi / d.h[c];
          if (gx >= d.bw[c] || gy >= d.bh[c]) return kJpegHuffCorrupt;
          base = (long long)d.coef_off[c] + ((long long)gy * d.bw[c] + gx) * 64;
        }
        const unsigned long long e = (unsigned long long)base + (unsigned)zigzag(k);
        if (k > 63 || e >= d.total_coefs) return kJpegHuffCorrupt;
        coef[e] = (int16_t)val;
      }
      ++k;
    }
    if (k >= 64) {
      // block done: next block of the MCU
      if (kStrict && br.pos > p.bit_len) return kJpegHuffCorrupt;   // consumed bits the stream does not have
      k = 0;
      base = -1;
      ++nblk;
      if (++b >= p.bpm) b = 0;
      c = b < n0 ? 0 : (b < n1 ? 1 : 2);
      if (kStrict && first_block + nblk >= p.total_blocks) break;   // what follows the last block is ignored
    }
  }
  pos = br.pos;
  return kJpegHuffOk;
}

JH_HD inline uint32_t jpeg_par_limit(const JpegParCtx& x, uint32_t j) {
  const uint64_t e = (uint64_t)(j + 1u) * x.sub_bits;
  return e < x.p->bit_len ? (uint32_t)e : x.p->bit_len;
}

JH_HD inline void jpeg_par_init(const JpegParCtx& x, uint32_t t, uint32_t T) {
  for (uint32_t j = t; j < x.nsub; j += T) {
    x.st[j] = kJpegParChanged;                  // (rel 0, k 0, b 0), to be decoded
    x.st[x.nsub + j] = 0;
  }
}

// One round reading entry buffer `cur` and writing the other one; true: this
// thread handed on an entry that differs from the one its successor had.
JH_HD inline bool jpeg_par_round(const JpegParCtx& x, int cur, uint32_t t, uint32_t T) {
  using namespace jpeg_huff_detail;
  const uint32_t n = x.nsub;
  const uint32_t* ent = x.st + (cur ? n : 0u);
  uint32_t* nxt = x.st + (cur ? 0u : n);
  bool any = false;
  for (uint32_t j = t; j < n; j += T) {
    const uint32_t e = ent[j];
    const uint32_t old = j + 1u < n ? ent[j + 1u] & ~kJpegParChanged : 0u;
    uint32_t out = old;                         // not decoded again: the exit it handed on last round
    if (e & kJpegParChanged) {
      uint32_t pos = j * x.sub_bits + (e & 255u), nblk = 0;
      int k = (int)((e >> 8) & 63u), b = (int)((e >> 16) & 63u);
      if (b >= x.p->bpm) b = 0;
      uint32_t dc[3] = {0u, 0u, 0u};
      const uint32_t limit = jpeg_par_limit(x, j);
      jpeg_par_lane<false>(*x.d, *x.p, x.words, *x.set, limit, pos, k, b, nblk, dc, 0u, nullptr);
      x.st[2u * n + j] = nblk;
      x.st[3u * n + j] = dc[0];
      x.st[4u * n + j] = dc[1];
      x.st[5u * n + j] = dc[2];
      out = par_pack((pos - limit) & 255u, k, b);   // j + 1 < n: limit = (j + 1) * S <= pos < limit + 31
    }
    if (j + 1u < n) {
      if (out != old) {
        out |= kJpegParChanged;
        any = true;
      }
      nxt[j + 1u] = out;
    }
    if (j == 0) nxt[0] = 0;                     // the true start: decoded once, in the first round
  }
  return any;
}

// Sums of blocks and DC differences over this thread's contiguous share of the sub-streams.
JH_HD inline void jpeg_par_range(const JpegParCtx& x, uint32_t t, uint32_t T, uint32_t* lo, uint32_t* hi) {
  const uint32_t per = x.nsub / T + (x.nsub % T ? 1u : 0u);
  const uint64_t a = (uint64_t)t * per, b = a + per;
  *lo = a < x.nsub ? (uint32_t)a : x.nsub;
  *hi = b < x.nsub ? (uint32_t)b : x.nsub;
}

JH_HD inline void jpeg_par_partial(const JpegParCtx& x, uint32_t t, uint32_t T, uint32_t part[4]) {
  uint32_t lo, hi;
  jpeg_par_range(x, t, T, &lo, &hi);
  part[0] = part[1] = part[2] = part[3] = 0u;
  for (uint32_t j = lo; j < hi; ++j)
    for (uint32_t q = 0; q < 4u; ++q) part[q] += x.st[(2u + q) * x.nsub + j];
}

// base[]: the sums of the threads before t.  Turns this thread's share into exclusive prefixes.
JH_HD inline void jpeg_par_scan(const JpegParCtx& x, uint32_t t, uint32_t T, const uint32_t base[4]) {
  uint32_t lo, hi;
  jpeg_par_range(x, t, T, &lo, &hi);
  uint32_t run[4] = {base[0], base[1], base[2], base[3]};
  for (uint32_t j = lo; j < hi; ++j)
    for (uint32_t q = 0; q < 4u; ++q) {
      uint32_t* w = &x.st[(2u + q) * x.nsub + j];
      const uint32_t v = *w;
      *w = run[q];
      run[q] += v;
    }
}

// The write pass from the converged entries in buffer `cur`; kJpegHuffCorrupt if one of this thread's lanes is refused.
JH_HD inline int jpeg_par_write(const JpegParCtx& x, int cur, uint32_t t, uint32_t T) {
  const uint32_t n = x.nsub;
  const uint32_t* ent = x.st + (cur ? n : 0u);
  int status = kJpegHuffOk;
  for (uint32_t j = t; j < n; j += T) {
    const uint32_t first = x.st[2u * n + j];
    if (first >= x.p->total_blocks) continue;   // after the scan's last block
    const uint32_t e = ent[j];
    uint32_t pos = j * x.sub_bits + (e & 255u), nblk = 0;
    int k = (int)((e >> 8) & 63u), b = (int)((e >> 16) & 63u);
    if (b >= x.p->bpm) b = 0;
    uint32_t dc[3] = {x.st[3u * n + j], x.st[4u * n + j], x.st[5u * n + j]};
    if (jpeg_par_lane<true>(*x.d, *x.p, x.words, *x.set, jpeg_par_limit(x, j), pos, k, b, nblk, dc, first, x.coef) !=
        kJpegHuffOk)
      status = kJpegHuffCorrupt;
  }
  return status;
}

}  // namespace idunno
