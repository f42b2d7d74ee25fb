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
//
// Which files are taken beyond 8-bit baseline 4:4:4 / 4:2:2 / 4:2:0 YCbCr or grey is the caller's
// choice: JpegOptions below.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../jpeg_huff_prog.h"

namespace idunno {

enum JpegStatus : int {
  JPEG_OK = 0,
  JPEG_EMPTY = 1,                // no bytes at all
  JPEG_NOT_JPEG = 2,             // no SOI marker (a PNG, ...)
  JPEG_CORRUPT = 3,              // truncation, bad code / marker / table, index past 63, DC overflow
  JPEG_UNSUPPORTED_PROGRESSIVE = 4,
  JPEG_UNSUPPORTED_ARITHMETIC = 5,
  JPEG_UNSUPPORTED_PRECISION = 6,   // 12-bit samples
  JPEG_UNSUPPORTED_COMPONENTS = 7,  // 4 components (CMYK / YCCK), or 2; with native_colorspace: 2, or 4 with an Adobe transform not 0 / 2
  JPEG_UNSUPPORTED_QUANT16 = 8,     // 16-bit quantisation tables
  JPEG_UNSUPPORTED_SAMPLING = 9,    // not 4:4:4 / 4:2:2 (2x1) / 4:2:0 (2x2); with native_sampling: nor 4:4:0 (1x2) / 4:1:1 (4x1); 4 components not all 1x1
  JPEG_UNSUPPORTED_SIZE = 10,       // above 4096 x 4096
  JPEG_UNSUPPORTED_MULTISCAN = 11,  // baseline with one scan per component; progressive above kJpegProgMaxScans
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
  int ncomp;           // 1 or 3; with native_colorspace also 4
  int hmax, vmax;
  int mode;            // chroma layout: 0 as luma, 1 half width (h2v1), 2 half width and height (h2v2);
                       // with native_sampling also 3 half height (h1v2, 4:4:0), 4 quarter width (h4v1, 4:1:1)
  int mcux, mcuy;      // MCU grid
  int restart_interval;
  uint32_t total_coefs;   // int16 elements the coefficient buffer must hold
  uint32_t scan_pos;      // byte offset of the entropy-coded data
  JpegComp comp[3];       // components 0..2; the fourth: comp_k below, at(c) reaches all four
  int progressive;        // 1: an SOF2 frame, accepted because the caller asked for native progressive decoding
  int nscans;             // its scans (1 for a baseline file)
  int colorspace;         // what the samples are: 0 YCbCr or grey, 1 RGB, 2 CMYK, 3 YCCK; always 0 without native_colorspace
  JpegComp comp_k;        // the fourth component (K of CMYK / YCCK): behind the ints, so that every field in front of
                          // it keeps the offset it has in the header rows callers read (mode, progressive)
  JpegComp& at(int c) { return c < 3 ? comp[c] : comp_k; }
  const JpegComp& at(int c) const { return c < 3 ? comp[c] : comp_k; }
};

// The scan script of a progressive file, in the form jpeg_huff_prog.h decodes: what
// the marker walk over the whole file (every SOS up to EOI) found.
struct JpegProgScript {
  std::vector<JpegProgScan> scans;     // byte_off relative to first_pos; table indices into tabs
  std::vector<JpegHuffTab> tabs;       // the tables in effect at some SOS, identical ones once
  std::vector<std::string> tab_keys;   // their DHT payloads (class, counts, symbols): what "identical" means
  uint32_t first_pos = 0;              // byte offset of the first scan's entropy-coded data in the file
};

// What a caller takes beyond the default; every member is an opt-in.  One value goes from the
// Python bindings through the parser, the host decoder, the packer and the descriptor checks, so
// that all of them agree on which files a batch may hold.
struct JpegOptions {
  // An SOF2 frame of a supported layout is not refused with JPEG_UNSUPPORTED_PROGRESSIVE: the
  // marker walk goes on over every scan up to EOI.  It refuses as JPEG_CORRUPT a scan with
  // Ss == 0 and Se != 0, an AC scan of more than one component, Se > 63, Ss > Se, Al > 13, a
  // refinement with Ah != Al + 1, a scan that uses an undefined table and a file without EOI;
  // more than kJpegProgMaxScans scans are JPEG_UNSUPPORTED_MULTISCAN.  A component's quantisation
  // table is the one in its slot at that component's first scan.  The host decoder runs the scan
  // core of ../jpeg_huff_prog.h, the packer gives the file gpu == 3, and the descriptor checks
  // take gpu == 3 entries (their scans: jpeg_huff_prog_check).
  bool native_progressive = false;
  // Packer and descriptor checks only (the parser and the host decoder ignore it): a baseline file
  // with a restart interval whose RSTn markers the packer finds gets gpu == 4 and one JpegRstItem
  // per interval, and the checks take gpu == 4 entries (their items: jpeg_huff_rst_check).
  bool restart_intervals = false;
  // A 3-component frame whose chroma components are both 1x1 and whose luma is 1x2 (4:4:0) or
  // 4x1 (4:1:1) is accepted as mode 3 or 4 and laid out like every other file of its kind (gpu 1
  // to 4); every other layout beyond modes 0..2 stays JPEG_UNSUPPORTED_SAMPLING.  Without it the
  // descriptor checks refuse an entry with those luma factors, which only a batch planned with
  // it holds.
  bool native_sampling = false;
  // The colour model is read as libjpeg reads it.  Three components: YCbCr when a JFIF APP0 was
  // seen; else, when an Adobe APP14 was seen (at least 12 bytes, starting with "Adobe"), RGB for
  // its transform byte 0 and YCbCr otherwise; else RGB for the component ids 'R','G','B' and
  // YCbCr for anything else.  Four components, all sampled 1x1 (mode 0; any other sampling is
  // JPEG_UNSUPPORTED_SAMPLING), baseline or progressive: CMYK without an Adobe segment or with
  // transform 0, YCCK with transform 2, JPEG_UNSUPPORTED_COMPONENTS for any other transform.
  // Without it hdr->colorspace is 0, every 3-component file is decoded as YCbCr downstream, an
  // RGB-coded one included, and a 4-component file is refused.  A 4-component file gets gpu == 1,
  // or gpu == 3 when progressive, whatever par_sub_bits and restart_intervals say (the sub-stream
  // and interval kernels keep to one and three components); RGB-coded files are laid out like
  // their YCbCr twins.  Without it the descriptor checks refuse a 4-component entry.
  bool native_colorspace = false;
};

// Parses the markers up to and including SOS, taking what opt admits (restart_intervals plays no
// part here).  Fills *hdr on JPEG_OK.  Of a progressive file the walk goes on over every scan up to
// EOI (hdr->progressive, hdr->nscans); *script, when given, receives the scan script.
int jpeg_parse_header(const uint8_t* data, size_t n, JpegHeader* hdr, const JpegOptions& opt = {},
                      JpegProgScript* script = nullptr);

// The frame layout of *hdr in a JpegHuffDesc (ncomp, MCU grid, per component
// sampling, padded grid, own grid, coefficient offsets, total_coefs): what
// jpeg_prog_decode_scan reads besides the byte span.
void jpeg_prog_frame_desc(const JpegHeader& hdr, JpegHuffDesc* d);

// Parses and decodes one image into out[0, out_cap) (int16 elements).  Never
// reads outside data[0, n) nor writes outside out[0, out_cap).  opt: as for
// jpeg_parse_header; a progressive file is decoded with the core of jpeg_huff_prog.h
// on a word-aligned copy of its scans, baseline files as without the option.
int jpeg_decode(const uint8_t* data, size_t n, JpegHeader* hdr, int16_t* out, size_t out_cap,
                const JpegOptions& opt = {});

// Decodes n images on a pool of `nthreads` std::threads (never derived from
// the machine's CPU count).  Image i with data[i] == nullptr is skipped with
// JPEG_EMPTY.  status[i] and hdr[i] are written for every i.
void jpeg_decode_batch(int n, const uint8_t* const* data, const size_t* len, JpegHeader* hdr,
                       int16_t* const* out, const size_t* out_cap, int* status, int nthreads = 8,
                       const JpegOptions& opt = {});

}  // namespace idunno
