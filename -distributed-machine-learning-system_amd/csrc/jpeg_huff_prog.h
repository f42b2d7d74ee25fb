// Progressive JPEG Huffman decode of one scan of one image, shared by the host
// decoder (runtime/jpeg_entropy.cpp, progressive="native"), the device kernel
// (kernels/jpeg_entropy.hip jpeg_entropy_prog_kernel, one lane per image) and the
// stand-alone checks (csrc/tests/jpeg_prog_checks.cpp).
//
// Host/device-pure like jpeg_huff_core.h: no torch, no HIP runtime calls, builds
// with --offload-host-only.  The caller hands it one image as the packer
// (runtime/jpeg_huff_pack.cpp, gpu == 3) laid it out:
//   * words: the file from the first scan's entropy-coded data to its end (the
//     later scans' DHT / SOS segments included: the reader stops at each marker),
//     4-byte aligned, zero-padded to kJpegHuffBytePad,
//   * scans: one JpegProgScan per SOS, in file order; byte_off is where the scan's
//     data starts inside the span,
//   * tabs:  single Huffman tables (a progressive file defines new ones before
//     almost every scan, so whole JpegHuffSets would multiply the upload),
//   * coef:  the image's own int16 span, zeroed by the caller, layout as
//     jpeg_entropy.h documents it.  A progressive file holds the same quantised
//     coefficients as its baseline twin, spread over scans by spectral band
//     (Ss..Se) and bit plane (Ah / Al).
//
// The rules (ITU-T T.81 annex G, as libjpeg's jdphuff.c applies them):
//   * a scan of one component walks that component's own block grid
//     gw x gh = ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8), NOT the
//     padded grid bw x bh of the interleaved MCUs, and its restart interval
//     counts blocks; a scan of several components (DC only) walks MCUs as the
//     baseline decoder does,
//   * first passes store value << Al; DC refinement ORs one bit in; AC
//     refinement reads one correction bit for every coefficient of the band that
//     is already nonzero (+-(1 << Al) away from zero where that bit is clear) and
//     places each new +-(1 << Al) after r still-zero positions,
//   * an EOB run spans blocks and is dropped at a restart; in a refinement scan
//     the blocks inside a run still read their correction bits.
// Arbitrary bytes and arbitrary scan descriptors give JPEG_OK or JPEG_CORRUPT,
// never an access outside the two spans: every store and read-modify-write is
// checked (zigzag index <= Se <= 63, block inside the component's grid, element
// inside the span), every value written fits int16, and every loop is bounded by
// the scan: blocks x (band length + 1) symbol trips, each followed by at most a
// band's length of correction bits.
#pragma once
#include <cstdint>

#include "jpeg_huff_core.h"

namespace idunno {

// Scans one file may hold.  libjpeg's default script (Pillow, jpegtran
// -progressive) has 10 scans for colour and 6 for grey, mozjpeg's scripts up to
// 12; 32 leaves room for hand-written scripts and bounds a corrupt file's
// decode time to 32 passes over its blocks.  Files above it: multiscan fallback.
constexpr int kJpegProgMaxScans = 32;

struct JpegProgScan {
  uint32_t byte_off;          // first entropy-coded byte of the scan inside the image's byte span
  int32_t ncomp;              // components in the scan, 1..4; more than one: an interleaved DC scan
  int32_t comp[4];            // their indices in the frame, ascending
  int32_t ss, se, ah, al;
  int32_t restart_interval;   // in effect at this SOS: MCUs (interleaved) or blocks (one component); 0: none
  int32_t dc_tab[4];          // per scan component: its DC table in the table buffer (DC first scans only), else -1
  int32_t ac_tab;             // the AC table (AC scans only), else -1
};

namespace jpeg_huff_detail {

// One block of the scan's component: where it lies and what a checked access needs.
struct ProgBlock {
  unsigned long long e0;      // first element of the block in the span
  uint32_t total;             // elements of the span
  int se;                     // last zigzag index the scan may touch
  // element of zigzag index k, or false: outside the band or the span
  JH_HD bool at(int k, unsigned long long* e) const {
    if (k < 0 || k > se || se > 63) return false;
    *e = e0 + (unsigned)zigzag(k);
    return *e < total;
  }
};

JH_HD inline bool fits16(int v) { return v >= -32768 && v <= 32767; }

// Bit k set: the coefficient of zigzag index k of the block at blk[0, 64) is nonzero.
// 64 independent loads at fixed offsets (a refinement scan asks "is it nonzero" for every
// position of the band: one dependent load each would make the scan wait for memory
// 63 times per block) and no indexed local array.
JH_HD inline uint64_t prog_nonzero_mask(const int16_t* blk) {
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < 64; ++k) m |= (uint64_t)(blk[zigzag(k)] != 0) << k;
  return m;
}

// one correction bit for the already nonzero coefficient at e
JH_HD inline bool prog_correct(Bits& br, int16_t* coef, unsigned long long e, int p1) {
  const unsigned bit = br.peek(1);
  br.skip(1);
  if (!bit) return true;
  const int v = coef[e];
  if ((v & p1) != 0) return true;            // that bit is set already
  const int nv = v >= 0 ? v + p1 : v - p1;
  if (!fits16(nv)) return false;
  coef[e] = (int16_t)nv;
  return true;
}

// DC scan, first (ah == 0) or refinement: one block per trip, the position (unit,
// component of the scan, block in the MCU) carried as state like jpeg_huff_decode_scan
JH_HD inline int prog_dc_scan(const JpegHuffDesc& d, const JpegProgScan& s, Bits& br, const JpegHuffTab* tabs,
                              int16_t* coef, long long* trips) {
  const bool inter = s.ncomp > 1;
  const int c0 = s.comp[0];
  const int nux = inter ? d.mcux : d.gw[c0], nuy = inter ? d.mcuy : d.gh[c0];
  long long nblk = 0;
  for (int q = 0; q < s.ncomp; ++q) nblk += inter ? (long long)d.mcux * d.mcuy * d.h[s.comp[q]] * d.v[s.comp[q]]
                                                  : (long long)nux * nuy;
  const int ri = s.restart_interval;
  const int p1 = 1 << s.al;
  int left = ri, rst = 0;
  int pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;
  int ux = 0, uy = 0, q = 0, bx = 0, by = 0;
  // the current component's layout and table
  int c = c0;
  int ch = inter ? d.h[c] : 1, cv = inter ? d.v[c] : 1;
  int lw = inter ? d.bw[c] : d.gw[c], lh = inter ? d.bh[c] : d.gh[c], cbw = d.bw[c];
  uint32_t coff = d.coef_off[c];
  const JpegHuffTab* dct = s.ah == 0 ? &tabs[s.dc_tab[0]] : nullptr;
  for (long long it = 0; it < nblk; ++it) {
    if (trips != nullptr) ++*trips;
    const int gx = ux * ch + bx, gy = uy * cv + by;
    const unsigned long long e = (unsigned long long)coff + ((unsigned long long)gy * (unsigned)cbw + (unsigned)gx) * 64ull;
    if (gx >= lw || gy >= lh || gx >= cbw || e >= d.total_coefs) return kJpegHuffCorrupt;
    if (br.nbits < 32) br.fill();
    if (s.ah == 0) {
      const int sym = symbol(br, *dct);
      if (sym < 0 || sym > 15) return kJpegHuffCorrupt;
      int pred = q == 0 ? pred0 : (q == 1 ? pred1 : (q == 2 ? pred2 : pred3));
      if (sym) pred += extend(br, sym);
      if (!fits16(pred)) return kJpegHuffCorrupt;
      if (q == 0) pred0 = pred;
      else if (q == 1) pred1 = pred;
      else if (q == 2) pred2 = pred;
      else pred3 = pred;
      const int val = pred * p1;                 // |pred| <= 2^15, al <= 13: no overflow of int
      if (!fits16(val)) return kJpegHuffCorrupt;
      coef[e] = (int16_t)val;
    } else {
      const unsigned bit = br.peek(1);
      br.skip(1);
      if (bit) coef[e] = (int16_t)(coef[e] | p1);
    }
    if (br.overrun) return kJpegHuffCorrupt;
    if (++bx == ch) {
      bx = 0;
      if (++by == cv) {
        by = 0;
        if (++q == s.ncomp) {
          q = 0;
          if (++ux == nux) {
            ux = 0;
            if (++uy == nuy) return kJpegHuffOk;
          }
          if (ri && --left == 0) {
            if (!br.restart(rst++)) return kJpegHuffCorrupt;
            pred0 = pred1 = pred2 = pred3 = 0;
            left = ri;
          }
        }
        if (inter) {
          c = s.comp[q];
          ch = d.h[c];
          cv = d.v[c];
          lw = cbw = d.bw[c];
          lh = d.bh[c];
          coff = d.coef_off[c];
          if (s.ah == 0) dct = &tabs[s.dc_tab[q]];
        }
      }
    }
  }
  return kJpegHuffCorrupt;   // not reached: the walk ends on the last block
}

// AC scan of one component, first (ah == 0) or refinement, over its own block grid
JH_HD inline int prog_ac_scan(const JpegHuffDesc& d, const JpegProgScan& s, Bits& br, const JpegHuffTab& act,
                              int16_t* coef, long long* trips) {
  const int c = s.comp[0];
  const int gw = d.gw[c], gh = d.gh[c], cbw = d.bw[c];
  const int ss = s.ss, se = s.se, band = se - ss + 1;
  const int p1 = 1 << s.al;
  const int ri = s.restart_interval;
  int left = ri, rst = 0;
  int eobrun = 0;
  ProgBlock b;
  b.total = d.total_coefs;
  b.se = se;
  if (gw > cbw) return kJpegHuffCorrupt;
  for (int gy = 0; gy < gh; ++gy) {
    for (int gx = 0; gx < gw; ++gx) {
      b.e0 = (unsigned long long)d.coef_off[c] + ((unsigned long long)gy * (unsigned)cbw + (unsigned)gx) * 64ull;
      unsigned long long e;
      int k = ss;
      if (trips != nullptr) ++*trips;
      if (s.ah == 0) {
        if (eobrun > 0) {
          --eobrun;
        } else {
          for (int trip = 0; k <= se; ++trip) {
            if (trip > band) return kJpegHuffCorrupt;         // not reached: every trip advances k or leaves
            if (trips != nullptr) ++*trips;
            if (br.nbits < 32) br.fill();
            const int sym = symbol(br, act);
            if (sym < 0) return kJpegHuffCorrupt;
            const int r = sym >> 4, sz = sym & 15;
            if (sz) {
              k += r;
              const int val = extend(br, sz) * p1;              // |extend| < 2^15, al <= 13
              if (!fits16(val) || !b.at(k, &e)) return kJpegHuffCorrupt;
              coef[e] = (int16_t)val;
              ++k;
            } else if (r == 15) {
              k += 16;                                          // ZRL
              if (k > se + 1) return kJpegHuffCorrupt;
            } else {
              eobrun = (1 << r) - 1;                            // this block is the run's first
              if (r) {
                eobrun += (int)br.peek(r);
                br.skip(r);
              }
              break;
            }
          }
        }
      } else {
        // the block's nonzero coefficients, kept up to date below: corrections move a value away
        // from zero, and a new coefficient is placed behind the position the walk has reached
        if (b.e0 + 64ull > (unsigned long long)b.total) return kJpegHuffCorrupt;
        uint64_t nz = prog_nonzero_mask(coef + b.e0);
        if (eobrun == 0) {
          for (int trip = 0; k <= se; ++trip) {
            if (trip > band) return kJpegHuffCorrupt;         // not reached: every trip advances k or leaves
            if (trips != nullptr) ++*trips;
            if (br.nbits < 32) br.fill();
            const int sym = symbol(br, act);
            if (sym < 0) return kJpegHuffCorrupt;
            int r = sym >> 4;
            const int sz = sym & 15;
            int nv = 0;
            if (sz) {
              if (sz != 1) return kJpegHuffCorrupt;             // a refinement adds one bit of magnitude
              nv = br.peek(1) ? p1 : -p1;
              br.skip(1);
            } else if (r != 15) {
              eobrun = 1 << r;                                  // this block included: its tail is corrected below
              if (r) {
                eobrun += (int)br.peek(r);
                br.skip(r);
              }
              break;
            }
            // pass r still-zero positions (a ZRL: 15 and the one after), correcting the nonzero ones on the way
            for (; k <= se; ++k) {
              if (trips != nullptr) ++*trips;
              if ((nz >> k) & 1u) {
                if (br.nbits < 32) br.fill();
                if (!b.at(k, &e) || !prog_correct(br, coef, e, p1)) return kJpegHuffCorrupt;
              } else if (--r < 0) {
                break;
              }
            }
            if (nv) {
              if (!b.at(k, &e)) return kJpegHuffCorrupt;        // the band ended before its place came
              coef[e] = (int16_t)nv;
              nz |= 1ull << k;
            }
            ++k;
          }
        }
        if (eobrun > 0) {
          // the rest of the band, k..se: only its nonzero coefficients read a bit
          uint64_t m = k <= se ? (nz >> k) << k : 0;
          if (se < 63) m &= (1ull << (se + 1)) - 1ull;
          while (m) {
            if (trips != nullptr) ++*trips;
            if (br.nbits < 32) br.fill();
            if (!b.at(__builtin_ctzll(m), &e) || !prog_correct(br, coef, e, p1)) return kJpegHuffCorrupt;
            m &= m - 1ull;
          }
          --eobrun;
        }
      }
      if (br.overrun) return kJpegHuffCorrupt;
      if (ri && --left == 0 && !(gy == gh - 1 && gx == gw - 1)) {
        if (!br.restart(rst++)) return kJpegHuffCorrupt;
        eobrun = 0;
        left = ri;
      }
    }
  }
  return kJpegHuffOk;
}

}  // namespace jpeg_huff_detail

// Decodes one scan of one image into its span.  d: the frame's layout and the byte
// span (gpu, set_idx, td, ta, restart_interval, scan_first, nscans are not read);
// tabs[0, ntabs): the table buffer s indexes.  trips (checks only, else nullptr):
// counts every loop trip, so that a caller can hold the total against the bound.
JH_HD inline int jpeg_prog_decode_scan(const JpegHuffDesc& d, const JpegProgScan& s, const uint32_t* words,
                                       const JpegHuffTab* tabs, int32_t ntabs, int16_t* coef,
                                       long long* trips = nullptr) {
  using namespace jpeg_huff_detail;
  if (d.ncomp != 1 && d.ncomp != 3 && d.ncomp != 4) return kJpegHuffCorrupt;
  if (d.mcux < 1 || d.mcuy < 1 || d.byte_len > d.byte_span || s.byte_off > d.byte_len) return kJpegHuffCorrupt;
  for (int c = 0; c < d.ncomp; ++c)
    if (d.h[c] < 1 || d.h[c] > 4 || d.v[c] < 1 || d.v[c] > 4 || d.bw[c] < 1 || d.bh[c] < 1 || d.gw[c] < 1 ||
        d.gh[c] < 1 || d.gw[c] > d.bw[c] || d.gh[c] > d.bh[c])
      return kJpegHuffCorrupt;
  if (s.ncomp < 1 || s.ncomp > d.ncomp) return kJpegHuffCorrupt;
  for (int q = 0; q < s.ncomp; ++q)
    if (s.comp[q] < 0 || s.comp[q] >= d.ncomp || (q > 0 && s.comp[q] <= s.comp[q - 1])) return kJpegHuffCorrupt;
  if (s.ss < 0 || s.se > 63 || s.ss > s.se || s.al < 0 || s.al > 13 || s.ah < 0 || (s.ah != 0 && s.ah != s.al + 1) ||
      s.restart_interval < 0)
    return kJpegHuffCorrupt;
  if (s.ss == 0 ? s.se != 0 : s.ncomp != 1) return kJpegHuffCorrupt;
  Bits br;
  br.init(words, d.byte_len);
  br.p = s.byte_off;
  if (s.ss == 0) {
    if (s.ah == 0)
      for (int q = 0; q < s.ncomp; ++q)
        if (s.dc_tab[q] < 0 || s.dc_tab[q] >= ntabs) return kJpegHuffCorrupt;
    return prog_dc_scan(d, s, br, tabs, coef, trips);
  }
  if (s.ac_tab < 0 || s.ac_tab >= ntabs) return kJpegHuffCorrupt;
  return prog_ac_scan(d, s, br, tabs[s.ac_tab], coef, trips);
}

// All scans of one image, in file order: what one lane of the kernel runs.
// scans[0, scans_total): the batch's scan descriptors, of which d names a range.
JH_HD inline int jpeg_prog_decode_image(const JpegHuffDesc& d, const JpegProgScan* scans, long long scans_total,
                                        const uint32_t* words, const JpegHuffTab* tabs, int32_t ntabs, int16_t* coef,
                                        long long* trips = nullptr) {
  if (d.nscans < 1 || d.nscans > kJpegProgMaxScans || d.scan_first < 0 ||
      (long long)d.scan_first + d.nscans > scans_total)
    return kJpegHuffCorrupt;
  for (int i = 0; i < d.nscans; ++i) {
    const int st = jpeg_prog_decode_scan(d, scans[d.scan_first + i], words, tabs, ntabs, coef, trips);
    if (st != kJpegHuffOk) return st;
  }
  return kJpegHuffOk;
}

}  // namespace idunno
