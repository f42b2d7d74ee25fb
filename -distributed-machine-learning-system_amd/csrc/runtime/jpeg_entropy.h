// Host-side baseline JPEG entropy decoder: bytes -> quantised DCT coefficients.
//
// Plain C++17 (no torch, no HIP) so that it builds stand-alone under sanitizers
// (csrc/tests/jpeg_checks.cpp).  The GPU does the rest (kernels/jpeg_decode.hip):
// dequantisation, IDCT, chroma upsampling, colour conversion, resize and crop.
//
// Output layout: per component, int16 coefficients NOT dequantised, natural
// (row-major u + 8 v) order, 64 per block, blocks row-major over the component's
// padded block grid (bw x bh = MCU grid x sampling factors); components follow
// each other at JpegComp::coef_off (in int16 elements).
#pragma once
#include <cstddef>
#include <cstdint>

namespace idunno {

enum JpegStatus : int {
  JPEG_OK = 0,
  JPEG_EMPTY = 1,                // no bytes at all
  JPEG_NOT_JPEG = 2,             // no SOI marker (a PNG, ...)
  JPEG_CORRUPT = 3,              // truncation, bad code / marker / table, index past 63, DC overflow
  JPEG_UNSUPPORTED_PROGRESSIVE = 4,
  JPEG_UNSUPPORTED_ARITHMETIC = 5,
  JPEG_UNSUPPORTED_PRECISION = 6,   // 12-bit samples
  JPEG_UNSUPPORTED_COMPONENTS = 7,  // 4 components (CMYK / YCCK), or 2
  JPEG_UNSUPPORTED_QUANT16 = 8,     // 16-bit quantisation tables
  JPEG_UNSUPPORTED_SAMPLING = 9,    // not 4:4:4 / 4:2:2 (2x1) / 4:2:0 (2x2)
  JPEG_UNSUPPORTED_SIZE = 10,       // above 4096 x 4096
  JPEG_UNSUPPORTED_MULTISCAN = 11,  // baseline with one scan per component
  JPEG_UNSUPPORTED_SOF = 12,        // lossless / hierarchical frames
  JPEG_BUFFER_TOO_SMALL = 13,       // caller's coefficient buffer < JpegHeader::total_coefs
  JPEG_STATUS_COUNT = 14,
};

const char* jpeg_status_name(int status);

constexpr int kJpegMaxDim = 4096;

struct JpegComp {
  int h, v;            // sampling factors (1 for a single-component image)
  int bw, bh;          // padded block grid
  int qidx;            // quantisation table slot
  uint32_t coef_off;   // first coefficient of this component, in int16 elements
  uint16_t q[64];      // quantisation table, natural order
};

struct JpegHeader {
  int W, H;
  int ncomp;           // 1 or 3
  int hmax, vmax;
  int mode;            // chroma layout: 0 as luma, 1 half width (h2v1), 2 half width and height (h2v2)
  int mcux, mcuy;      // MCU grid
  int restart_interval;
  uint32_t total_coefs;   // int16 elements the coefficient buffer must hold
  uint32_t scan_pos;      // byte offset of the entropy-coded data
  JpegComp comp[3];
};

// Parses the markers up to and including SOS.  Fills *hdr on JPEG_OK.
int jpeg_parse_header(const uint8_t* data, size_t n, JpegHeader* hdr);

// Parses and decodes one image into out[0, out_cap) (int16 elements).  Never
// reads outside data[0, n) nor writes outside out[0, out_cap).
int jpeg_decode(const uint8_t* data, size_t n, JpegHeader* hdr, int16_t* out, size_t out_cap);

// Decodes n images on a pool of `nthreads` std::threads (never derived from
// the machine's CPU count).  Image i with data[i] == nullptr is skipped with
// JPEG_EMPTY.  status[i] and hdr[i] are written for every i.
void jpeg_decode_batch(int n, const uint8_t* const* data, const size_t* len, JpegHeader* hdr,
                       int16_t* const* out, const size_t* out_cap, int* status, int nthreads = 8);

}  // namespace idunno
