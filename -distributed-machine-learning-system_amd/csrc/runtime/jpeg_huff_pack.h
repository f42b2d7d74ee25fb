// Host packer of the device entropy stage: turns a batch of JPEG files into what
// jpeg_huff_core.h decodes -- one contiguous byte buffer, one table buffer, one
// descriptor per image.  Plain C++17 like jpeg_entropy.cpp (no torch, no HIP), so
// it builds stand-alone under sanitizers (csrc/tests/jpeg_huff_core_checks.cpp).
//
// The marker parse is jpeg_parse_header's; the Huffman tables, which a
// JpegHeader does not keep, are read here from the DHT segments of a file that
// parse has already accepted.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../jpeg_huff_core.h"
#include "../jpeg_huff_par.h"
#include "../jpeg_huff_rst.h"
#include "jpeg_entropy.h"

namespace idunno {

struct JpegHuffBatch {
  std::vector<JpegHuffDesc> desc;   // one per entry, gpu == 0 where status != JPEG_OK
  std::vector<JpegHuffSet> sets;    // identical table sets share one entry
  int64_t byte_total = 0;           // bytes of the batch byte buffer
  int64_t coef_total = 0;           // int16 elements of the batch coefficient buffer
  // the sub-stream form (jpeg_huff_plan with par_sub_bits != 0), else empty / 0
  std::vector<JpegParDesc> par;     // one per entry, meaningful where desc[i].gpu == 2
  int64_t scratch_total = 0;        // uint32 elements of the batch scratch buffer
  // progressive files (jpeg_huff_plan with opt.native_progressive), else empty
  std::vector<JpegProgScan> scans;  // the scan scripts of the gpu == 3 entries, back to back
  std::vector<JpegHuffTab> tabs;    // the single tables those scans index; identical tables share one entry
  // restart-interval files (jpeg_huff_plan with opt.restart_intervals), else empty
  std::vector<JpegRstItem> rst_items;   // one per interval of the gpu == 4 entries, entry by entry, ascending
};

// Parses every entry (data[i] == nullptr: JPEG_EMPTY) and lays the batch out.
// status[i] and hdr[i] are what jpeg_parse_header gives; an accepted image gets
// its byte span at an aligned offset and its coefficients after its predecessors'.
// par_sub_bits != 0 (a multiple of 32, the sub-stream size of jpeg_huff_par.h) lays
// the batch out for the sub-stream kernel as well: an accepted image without a
// restart interval whose scan is shorter than kJpegParMaxBits gets gpu == 2, a byte
// span sized for its de-stuffed words, a JpegParDesc and a scratch span; every
// other accepted image keeps gpu == 1 and the stuffed layout of the one-lane kernel.
// opt (JpegOptions, jpeg_entropy.h) goes to jpeg_parse_header and decides which of the further
// layouts the batch may hold:
// gpu == 3, a progressive file, in either form: its byte span is the file from the first scan's
// data to the end in the stuffed layout of gpu == 1, and it names a range of out->scans
// (jpeg_huff_prog.h), whose tables are entries of out->tabs.
// gpu == 4, with opt.restart_intervals: an accepted baseline file with a restart interval is
// scanned once from scan_pos by the byte rules of jpeg_huff_detail::Bits::fill (FF 00 data, FF FF
// fill, any other FF xx a marker) for the byte offset after each in-sequence RSTn, up to
// the first other marker, an out-of-sequence RSTn or the end.  With at least
// ceil(mcux * mcuy / ri) - 1 markers (later ones are ignored, as the serial decoder
// ignores what follows the last MCU) it gets gpu == 4 in either form: the stuffed layout
// of gpu == 1 and one JpegRstItem per interval in out->rst_items (jpeg_huff_rst.h); a
// restart interval of at least the MCU count needs no marker and is one item.  With
// fewer markers the serial decoder will refuse the file: it keeps gpu == 1 and the
// one-lane kernel gives the verdict.  gpu == 2 and gpu == 3 entries are untouched.
void jpeg_huff_plan(int n, const uint8_t* const* data, const size_t* len, JpegHeader* hdr, int* status,
                    JpegHuffBatch* out, uint32_t par_sub_bits = 0, const JpegOptions& opt = {});

// Copies the entropy-coded bytes of every gpu entry to dst[0, byte_total) and
// zeroes the padding between them.  A gpu == 2 entry gets its de-stuffed words
// instead: FF 00 -> FF, fill bytes dropped, cut at the first marker (the rules of
// jpeg_huff_detail::Bits::fill), four bytes per word, most significant first.
void jpeg_huff_copy_bytes(const JpegHuffBatch& b, const uint8_t* const* data, const size_t* len, uint8_t* dst);

// Every descriptor against the three buffers it indexes (byte_cap bytes, nsets
// table sets, coef_cap int16 elements): nullptr when every span lies inside them
// and the layout inside each span is consistent, else what is wrong.  Run before
// a launch.
// opt: what the batch was planned with; an entry that only another JpegOptions admits is refused.
const char* jpeg_huff_check(const JpegHuffDesc* desc, int n, int64_t byte_cap, int64_t nsets, int64_t coef_cap,
                            const JpegOptions& opt = {});

// The same for a batch planned with par_sub_bits: gpu == 1 entries as above, gpu == 2
// entries also against their JpegParDesc and the scratch buffer (scratch_cap uint32
// elements, kJpegParStateWords per sub-stream of sub_bits bits).
const char* jpeg_huff_par_check(const JpegHuffDesc* desc, const JpegParDesc* par, int n, int64_t byte_cap,
                                int64_t nsets, int64_t coef_cap, int64_t scratch_cap, uint32_t sub_bits,
                                const JpegOptions& opt = {});

// The gpu == 3 entries against the scan buffer (nscans JpegProgScan) and the table
// buffer (ntabs JpegHuffTab) the progressive kernel will get: every image's scan
// range inside the scan buffer, every scan's offset inside the image's byte span,
// its parameters within what the core accepts, every table index it will use inside
// the table buffer.  Run next to jpeg_huff_check with opt.native_progressive before a launch.
const char* jpeg_huff_prog_check(const JpegHuffDesc* desc, int n, const JpegProgScan* scans, int64_t nscans,
                                 int64_t ntabs);

// The work items of the interval kernel against the descriptors: every item's entry a
// gpu == 4 entry, byte_begin < byte_len, mcu_first == index * restart_interval <
// mcux * mcuy; the items of one entry contiguous, ascending and complete (every gpu == 4
// entry has all ceil(mcux * mcuy / ri) of them, entries ascending); nitems < 2^31.  Run
// next to jpeg_huff_check with opt.restart_intervals before a launch.
const char* jpeg_huff_rst_check(const JpegHuffDesc* desc, int n, const JpegRstItem* items, int64_t nitems);

}  // namespace idunno
