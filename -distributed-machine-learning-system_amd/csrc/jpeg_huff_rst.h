// Baseline JPEG Huffman decode of one restart interval, shared by the device
// kernel (kernels/jpeg_entropy.hip: jpeg_entropy_rst_kernel, one lane per
// interval) and the host (csrc/tests/jpeg_huff_rst_checks.cpp, differential
// against runtime/jpeg_entropy.cpp).
//
// Host/device-pure like jpeg_huff_core.h, whose reader, symbol lookup, sign
// extension and zigzag table it uses.  A file with a restart interval (DRI, RSTn
// markers in the scan) is parallel by construction: after every RSTn the reader
// is byte-aligned, the DC predictors are zero and the MCU number is known.  The
// packer (runtime/jpeg_huff_pack.cpp, restart_intervals) finds the markers with
// one byte scan and hands out one JpegRstItem per interval; each item is decoded
// by jpeg_huff_decode_scan's own loop, started in the state the serial decoder
// has right after that marker:
//   * the reader at byte_begin of the image's stuffed span, its end still the
//     image's byte_len, so it stops on the next marker by the serial rule,
//   * the predictors at zero, the position at MCU mcu_first,
//   * min(restart_interval, mcux * mcuy - mcu_first) MCUs to decode.
// An interval that is not the scan's last ends with the very Bits::restart call
// the serial loop makes (less than a whole data byte left, fill FFs skipped, the
// marker RST(rst_index mod 8)); the last one ends where the serial loop returns,
// whatever follows.  So every interval accepted <=> the serial decode accepted:
// interval k starts where the serial decoder stands if 0..k-1 were accepted, and
// the first interval to fail fails the serial decoder in the same state.  The
// coefficients are the serial decoder's, because intervals write disjoint blocks.
//
// Arbitrary bytes and arbitrary (byte_begin, mcu_first, rst_index) give JPEG_OK or
// JPEG_CORRUPT, never an access outside the two spans: the checks and bounds are
// those of the one-lane core (every store checked, overrun at every block end, 65
// symbols per block of the interval).
#pragma once
#include "jpeg_huff_core.h"

namespace idunno {

// One restart interval of a gpu == 4 entry: 16 bytes, a few KB per image at worst.
struct JpegRstItem {
  int32_t entry;          // index into the batch's JpegHuffDesc
  uint32_t byte_begin;    // first byte of the interval in the entry's byte span (after the RSTn in front of it)
  int32_t mcu_first;      // == index * restart_interval
  int32_t index;          // the interval's number in the scan; it ends with RST(index mod 8) unless it is the last
};

JH_HD inline int jpeg_huff_decode_interval(const JpegHuffDesc& d, const uint32_t* words, const JpegHuffSet& set,
                                           int16_t* coef, uint32_t byte_begin, int32_t mcu_first, int32_t rst_index) {
  using namespace jpeg_huff_detail;
  const int ncomp = d.ncomp;
  if (ncomp != 1 && ncomp != 3) return kJpegHuffCorrupt;
  if (d.mcux < 1 || d.mcuy < 1 || d.byte_len > d.byte_span) return kJpegHuffCorrupt;
  int bpm = 0;
  for (int c = 0; c < ncomp; ++c) {
    if (d.h[c] < 1 || d.h[c] > 4 || d.v[c] < 1 || d.v[c] > 4 || d.bw[c] < 1 || d.bh[c] < 1) return kJpegHuffCorrupt;
    if ((unsigned)d.td[c] > 3u || (unsigned)d.ta[c] > 3u) return kJpegHuffCorrupt;
    bpm += d.h[c] * d.v[c];
  }
  const int ri = d.restart_interval;
  const long long mcus = (long long)d.mcux * d.mcuy;
  if (ri < 1 || mcu_first < 0 || (long long)mcu_first >= mcus || rst_index < 0 || byte_begin > d.byte_len)
    return kJpegHuffCorrupt;
  const bool last = mcus - mcu_first <= (long long)ri;
  int left = last ? (int)(mcus - mcu_first) : ri;
  Bits br;
  br.init(words, d.byte_len);
  br.p = byte_begin;
  const uint32_t total = d.total_coefs;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int mx = mcu_first % d.mcux, my = mcu_first / d.mcux, c = 0, bx = 0, by = 0, k = 0;
  // the current component's layout and tables
  int ch = d.h[0], cv = d.v[0], cbw = d.bw[0], cbh = d.bh[0];
  uint32_t coff = d.coef_off[0];
  const JpegHuffTab* dct = &set.dc[d.td[0]];
  const JpegHuffTab* act = &set.ac[d.ta[0]];
  const long long limit = (long long)left * bpm * 65;
  for (long long it = 0; it < limit; ++it) {
    if (br.nbits < 32) br.fill();
    const int sym = symbol(br, k == 0 ? *dct : *act);
    if (sym < 0) return kJpegHuffCorrupt;
    int s = sym & 15;
    int val = 0;
    bool store = false;
    if (k == 0) {
      if (sym > 15) return kJpegHuffCorrupt;
      int pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
      if (s) pred += extend(br, s);
      if (pred < -32768 || pred > 32767) return kJpegHuffCorrupt;
      if (c == 0) pred0 = pred;
      else if (c == 1) pred1 = pred;
      else pred2 = pred;
      val = pred;
      store = true;
    } else {
      const int r = sym >> 4;
      if (s == 0) {
        if (r != 15) {
          k = 64;                                   // EOB
        } else {
          k += 16;                                  // ZRL
          if (k > 64) return kJpegHuffCorrupt;
        }
      } else {
        k += r;
        if (k > 63) return kJpegHuffCorrupt;
        val = extend(br, s);
        store = true;
      }
    }
    if (store) {
      const int gx = mx * ch + bx, gy = my * cv + by;
      const unsigned long long e = (unsigned long long)coff +
                                   ((unsigned long long)gy * (unsigned)cbw + (unsigned)gx) * 64ull + (unsigned)zigzag(k);
      if (k > 63 || gx >= cbw || gy >= cbh || e >= total) return kJpegHuffCorrupt;
      coef[e] = (int16_t)val;
      ++k;
    }
    if (k >= 64) {
      // block done: next block of the MCU, next component, next MCU
      if (br.overrun) return kJpegHuffCorrupt;
      k = 0;
      if (++bx == ch) {
        bx = 0;
        if (++by == cv) {
          by = 0;
          if (++c == ncomp) {
            c = 0;
            if (++mx == d.mcux) {
              mx = 0;
              ++my;
            }
            if (--left == 0) {
              // the interval's last MCU: the scan's end, or the marker the serial loop consumes here
              if (last) return kJpegHuffOk;
              return br.restart(rst_index) ? kJpegHuffOk : kJpegHuffCorrupt;
            }
          }
          ch = d.h[c];
          cv = d.v[c];
          cbw = d.bw[c];
          cbh = d.bh[c];
          coff = d.coef_off[c];
          dct = &set.dc[d.td[c]];
          act = &set.ac[d.ta[c]];
        }
      }
    }
  }
  return kJpegHuffCorrupt;   // not reached: every block ends within 65 symbols
}

}  // namespace idunno
