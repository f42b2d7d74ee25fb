// Baseline JPEG Huffman decode of one whole scan, shared by the device kernel
// (kernels/jpeg_entropy.hip, one lane per image) and the host (csrc/tests/
// jpeg_huff_core_checks.cpp, differential against runtime/jpeg_entropy.cpp).
//
// Host/device-pure like tile_math.h: no torch, no HIP runtime calls, builds with
// --offload-host-only.  The caller hands it one image as the packer
// (runtime/jpeg_huff_pack.cpp) laid it out:
//   * words: the entropy-coded bytes from JpegHeader::scan_pos to the end of the
//     file, 4-byte aligned, zero-padded to kJpegHuffBytePad; read only as whole
//     aligned 32-bit words below the padded length,
//   * set:   the 4 DC + 4 AC tables of the scan (undefined slots hold no code),
//   * coef:  the image's own int16 span (JpegHuffDesc::total_coefs elements,
//     zeroed by the caller), layout as jpeg_entropy.h documents it.
// Arbitrary bytes give JPEG_OK or JPEG_CORRUPT, never an access outside the two
// spans: every coefficient store is checked (zigzag index <= 63, block inside
// the component's grid, element inside the span), and the loop is bounded by 65
// symbols per block; past the end of data the reader yields zero bits, which
// the overrun flag turns into JPEG_CORRUPT.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define JH_HD __host__ __device__
#else
#define JH_HD
#endif

namespace idunno {

constexpr int kJpegHuffLookBits = 9;
constexpr int kJpegHuffBytePad = 4;       // byte spans are padded to a multiple of this (word loads)
constexpr int kJpegHuffByteAlign = 16;    // and start at a multiple of this in the batch buffer
constexpr int kJpegHuffOk = 0;            // == JPEG_OK
constexpr int kJpegHuffCorrupt = 3;       // == JPEG_CORRUPT (static_assert in jpeg_huff_pack.cpp)

struct JpegHuffTab {
  uint16_t look[1 << kJpegHuffLookBits];  // (length << 8) | symbol for codes of <= 9 bits, else 0
  int32_t maxcode[17];                    // largest code of each length, -1: none
  int32_t mincode[17];
  int32_t valptr[17];
  int32_t nvals;
  uint8_t vals[256];
};

struct JpegHuffSet {
  JpegHuffTab dc[4], ac[4];
};

// One per batch entry.  gpu == 0: not decoded on the device (nothing else is meaningful).
struct JpegHuffDesc {
  int64_t byte_off;        // first entropy-coded byte in the batch byte buffer (multiple of kJpegHuffByteAlign)
  int64_t coef_base;       // first coefficient in the batch coefficient buffer, int16 elements
  uint32_t byte_len;       // bytes from scan_pos to the end of the file
  uint32_t byte_span;      // byte_len rounded up to kJpegHuffBytePad: what the core may load
  uint32_t total_coefs;    // this image's coefficient span
  int32_t set_idx;         // its JpegHuffSet in the table buffer
  int32_t gpu;
  int32_t ncomp, mcux, mcuy, restart_interval;
  int32_t h[4], v[4], bw[4], bh[4], td[4], ta[4];   // four: CMYK / YCCK (one-lane and progressive kernels only)
  uint32_t coef_off[4];
  // gpu == 3 only (a progressive file, jpeg_huff_prog.h): each component's own block grid and
  // the image's range in the batch's JpegProgScan array; set_idx, td, ta, restart_interval unused
  int32_t gw[4], gh[4];
  int32_t scan_first, nscans;
};

namespace jpeg_huff_detail {

JH_HD inline int zigzag(int k) {
  const uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// MSB-first reader over [0, end) of an image's byte span.  Bytes come out of a
// one-word cache, so the stream is read with aligned 32-bit loads only.  FF 00 is
// a data byte FF, FF FF.. are fill bytes, FF xx stops the reader on the FF; from
// then on it feeds zero bits (`pad` counts those still in acc) and consuming one
// sets `overrun`.
struct Bits {
  const uint32_t* words;
  uint32_t p, end;
  uint32_t w, wpos;
  uint64_t acc;
  int nbits, pad;
  bool stopped, overrun;

  JH_HD void init(const uint32_t* words_, uint32_t end_) {
    words = words_;
    p = 0;
    end = end_;
    w = 0;
    wpos = 0xFFFFFFFFu;
    acc = 0;
    nbits = pad = 0;
    stopped = overrun = false;
  }
  // byte q of the span; the caller has checked q < end
  JH_HD unsigned byte(uint32_t q) {
    if ((q >> 2) != wpos) {
      wpos = q >> 2;
      w = words[wpos];
    }
    return (w >> (8u * (q & 3u))) & 255u;
  }
  JH_HD void fill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (!stopped) {
        if (p >= end) {
          stopped = true;
        } else {
          b = byte(p);
          if (b != 0xFFu) {
            ++p;
          } else if (p + 1 >= end) {
            stopped = true;
          } else {
            const unsigned b2 = byte(p + 1);
            if (b2 == 0xFFu) {
              ++p;                // fill byte: look again from the next FF
              continue;
            }
            if (b2 == 0x00u) p += 2;
            else stopped = true;  // a marker: stay on its FF
          }
        }
      }
      if (stopped) {
        b = 0;
        pad += 8;
      }
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  JH_HD unsigned peek(int k) const { return (unsigned)(acc >> (nbits - k)) & ((1u << k) - 1u); }
  JH_HD void skip(int k) {
    nbits -= k;
    if (nbits < pad) {
      overrun = true;
      pad = nbits;
    }
  }
  // byte-align and consume RST(idx mod 8); false: not there
  JH_HD bool restart(int idx) {
    if (nbits - pad >= 8) return false;   // whole data bytes in front of the marker
    acc = 0;
    nbits = pad = 0;
    stopped = false;
    if (p + 2 > end || byte(p) != 0xFFu) return false;
    while (p < end && byte(p) == 0xFFu) ++p;
    if (p >= end || byte(p) != 0xD0u + (unsigned)(idx & 7)) return false;
    ++p;
    return true;
  }
};

// a Huffman symbol, or -1 on a code the table does not hold; needs >= 16 bits in acc
// (B: Bits, or the plain-index reader of jpeg_huff_par.h)
template <class B>
JH_HD inline int symbol(B& br, const JpegHuffTab& t) {
  const unsigned e = t.look[br.peek(kJpegHuffLookBits)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  const unsigned c16 = br.peek(16);
  for (int l = kJpegHuffLookBits + 1; l <= 16; ++l) {
    const int32_t c = (int32_t)(c16 >> (16 - l));
    const int32_t mx = t.maxcode[l], mn = t.mincode[l];
    if (mx >= 0 && c <= mx && c >= mn) {
      const int idx = t.valptr[l] + (c - mn);
      if (idx < 0 || idx >= t.nvals || idx > 255) return -1;
      br.skip(l);
      return t.vals[idx];
    }
  }
  return -1;
}

// s in 1..15 magnitude bits -> signed value
template <class B>
JH_HD inline int extend(B& br, int s) {
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace jpeg_huff_detail

// Decodes the scan of one image.  One flat loop, one Huffman symbol per trip, the
// position (MCU, component, block in MCU, zigzag index) carried as state, so that
// lanes of a wave decoding different images stay on the same instructions across
// block, component and MCU boundaries.
JH_HD inline int jpeg_huff_decode_scan(const JpegHuffDesc& d, const uint32_t* words, const JpegHuffSet& set,
                                       int16_t* coef) {
  using namespace jpeg_huff_detail;
  const int ncomp = d.ncomp;
  if (ncomp != 1 && ncomp != 3 && ncomp != 4) return kJpegHuffCorrupt;
  if (d.mcux < 1 || d.mcuy < 1 || d.byte_len > d.byte_span) return kJpegHuffCorrupt;
  long long nblk = 0;
  for (int c = 0; c < ncomp; ++c) {
    if (d.h[c] < 1 || d.h[c] > 4 || d.v[c] < 1 || d.v[c] > 4 || d.bw[c] < 1 || d.bh[c] < 1) return kJpegHuffCorrupt;
    if ((unsigned)d.td[c] > 3u || (unsigned)d.ta[c] > 3u) return kJpegHuffCorrupt;
    nblk += (long long)d.mcux * d.mcuy * d.h[c] * d.v[c];
  }
  Bits br;
  br.init(words, d.byte_len);
  const uint32_t total = d.total_coefs;
  const int ri = d.restart_interval;
  int left = ri, rst = 0;
  int pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;
  int mx = 0, my = 0, c = 0, bx = 0, by = 0, k = 0;
  // the current component's layout and tables
  int ch = d.h[0], cv = d.v[0], cbw = d.bw[0], cbh = d.bh[0];
  uint32_t coff = d.coef_off[0];
  const JpegHuffTab* dct = &set.dc[d.td[0]];
  const JpegHuffTab* act = &set.ac[d.ta[0]];
  const long long limit = nblk * 65;
  for (long long it = 0; it < limit; ++it) {
    if (br.nbits < 32) br.fill();
    const int sym = symbol(br, k == 0 ? *dct : *act);
    if (sym < 0) return kJpegHuffCorrupt;
    int s = sym & 15;
    int val = 0;
    bool store = false;
    if (k == 0) {
      if (sym > 15) return kJpegHuffCorrupt;
      int pred = c == 0 ? pred0 : (c == 1 ? pred1 : (c == 2 ? pred2 : pred3));
      if (s) pred += extend(br, s);
      if (pred < -32768 || pred > 32767) return kJpegHuffCorrupt;
      if (c == 0) pred0 = pred;
      else if (c == 1) pred1 = pred;
      else if (c == 2) pred2 = pred;
      else pred3 = pred;
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
              if (++my == d.mcuy) return kJpegHuffOk;
            }
            if (ri && --left == 0) {
              if (!br.restart(rst++)) return kJpegHuffCorrupt;
              pred0 = pred1 = pred2 = pred3 = 0;
              left = ri;
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
