// Host packer of the device entropy stage (see jpeg_huff_pack.h).
#include "jpeg_huff_pack.h"

#include <cstring>
#include <map>
#include <string>

namespace idunno {

static_assert(kJpegHuffOk == JPEG_OK && kJpegHuffCorrupt == JPEG_CORRUPT, "core statuses are JpegStatus values");

namespace {

// The DHT payload of one table slot: 16 counts, then the symbols.
struct RawTab {
  bool defined = false;
  uint8_t counts[16];
  int nvals = 0;
  uint8_t vals[256];
};

struct RawSet {
  RawTab t[8];            // dc 0..3, ac 0..3
  int td[4], ta[4];
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Walks the segments of a file jpeg_parse_header accepted (so every length and
// every DHT payload has been validated) up to SOS at scan_pos; a later DHT of a
// slot replaces an earlier one.  false: the file is not what parse saw.
bool read_tables(const uint8_t* data, size_t n, const JpegHeader& hdr, RawSet* rs) {
  size_t pos = 2;
  while (pos + 2 <= n && pos < hdr.scan_pos) {
    if (data[pos] != 0xFF) return false;
    while (pos < n && data[pos] == 0xFF) ++pos;
    if (pos >= n) return false;
    const int m = data[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (pos + 2 > n) return false;
    const size_t L = (size_t)be16(data + pos);
    if (L < 2 || pos + L > n) return false;
    const uint8_t* seg = data + pos + 2;
    const size_t slen = L - 2;
    pos += L;
    if (m == 0xC4) {
      size_t p = 0;
      while (p < slen) {
        const int tc = seg[p] >> 4, th = seg[p] & 15;
        if (tc > 1 || th > 3 || p + 17 > slen) return false;
        RawTab& t = rs->t[4 * tc + th];
        int total = 0;
        for (int l = 0; l < 16; ++l) total += seg[p + 1 + l];
        if (total > 256 || p + 17 + (size_t)total > slen) return false;
        std::memcpy(t.counts, seg + p + 1, 16);
        std::memset(t.vals, 0, sizeof(t.vals));
        std::memcpy(t.vals, seg + p + 17, (size_t)total);
        t.nvals = total;
        t.defined = true;
        p += 17 + (size_t)total;
      }
    } else if (m == 0xDA) {
      if (pos != hdr.scan_pos || slen != (size_t)(4 + 2 * hdr.ncomp) || seg[0] != hdr.ncomp) return false;
      for (int c = 0; c < hdr.ncomp; ++c) {
        rs->td[c] = seg[2 + 2 * c] >> 4;
        rs->ta[c] = seg[2 + 2 * c] & 15;
        if (rs->td[c] > 3 || rs->ta[c] > 3) return false;
        if (!rs->t[rs->td[c]].defined || !rs->t[4 + rs->ta[c]].defined) return false;
      }
      return true;
    }
  }
  return false;
}

// canonical code tables of one slot, in the core's form; false: counts no code can have
bool build_tab(const RawTab& r, JpegHuffTab* t) {
  std::memset(t, 0, sizeof(*t));
  for (int l = 0; l <= 16; ++l) t->maxcode[l] = -1;
  if (!r.defined) return true;          // holds no code: every lookup fails
  std::memcpy(t->vals, r.vals, sizeof(t->vals));
  t->nvals = r.nvals;
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = r.counts[l - 1];
    if (code + cnt > (1 << l)) return false;
    t->valptr[l] = k;
    t->mincode[l] = code;
    t->maxcode[l] = cnt ? code + cnt - 1 : -1;
    if (l <= kJpegHuffLookBits) {
      const int rep = 1 << (kJpegHuffLookBits - l);
      for (int i = 0; i < cnt; ++i)
        for (int j = 0; j < rep; ++j) t->look[(code + i) * rep + j] = (uint16_t)((l << 8) | r.vals[k + i]);
    }
    k += cnt;
    code = (code + cnt) << 1;
  }
  return true;
}

std::string set_key(const RawSet& rs) {
  std::string key;
  for (const RawTab& t : rs.t) {
    key.push_back(t.defined ? 1 : 0);
    if (!t.defined) continue;
    key.append(reinterpret_cast<const char*>(t.counts), 16);
    key.append(reinterpret_cast<const char*>(t.vals), (size_t)t.nvals);
  }
  return key;
}

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// The data bytes of src[0, n) as jpeg_huff_detail::Bits::fill yields them, up to the
// first marker, a lone trailing FF or the end; returns their number.  dst (or
// nullptr: count only) receives byte i at (i & ~3) | (3 - (i & 3)): words whose most
// significant byte comes first; never more than cap bytes.
size_t destuff(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) {
  size_t p = 0, k = 0;
  while (p < n && k < cap) {
    unsigned b = src[p];
    if (b != 0xFFu) {
      ++p;
    } else if (p + 1 >= n) {
      break;
    } else if (src[p + 1] == 0xFFu) {
      ++p;                          // fill byte: look again from the next FF
      continue;
    } else if (src[p + 1] == 0x00u) {
      p += 2;
    } else {
      break;                        // a marker
    }
    if (dst != nullptr) dst[(k & ~(size_t)3) | (3u - (k & 3u))] = (uint8_t)b;
    ++k;
  }
  return k;
}

}  // namespace

void jpeg_huff_plan(int n, const uint8_t* const* data, const size_t* len, JpegHeader* hdr, int* status,
                    JpegHuffBatch* out, uint32_t par_sub_bits, const JpegOptions& opt) {
  out->desc.assign((size_t)n, JpegHuffDesc{});
  out->sets.clear();
  out->scans.clear();
  out->tabs.clear();
  out->rst_items.clear();
  std::vector<uint32_t> begins;
  std::map<std::string, int> seen_tabs;
  JpegProgScript script;
  out->byte_total = out->coef_total = out->scratch_total = 0;
  out->par.clear();
  if (par_sub_bits) out->par.assign((size_t)n, JpegParDesc{});
  std::map<std::string, int> seen;
  std::vector<RawSet> rsv(1);                 // ~2 KB: off the stack
  for (int i = 0; i < n; ++i) {
    JpegHuffDesc& d = out->desc[(size_t)i];
    std::memset(&hdr[i], 0, sizeof(hdr[i]));
    if (data[i] == nullptr || len[i] == 0) {
      status[i] = JPEG_EMPTY;
      continue;
    }
    status[i] = jpeg_parse_header(data[i], len[i], &hdr[i], opt, &script);
    if (status[i] != JPEG_OK) continue;
    const JpegHeader& h = hdr[i];
    if (h.progressive) {
      // the whole file from the first scan's data on, stuffed as it is; one descriptor per scan,
      // its tables one JpegHuffTab at a time, identical ones shared across the batch
      if (script.first_pos > len[i] || len[i] - script.first_pos > 0xFFFFFFF0u || script.scans.empty() ||
          out->scans.size() + script.scans.size() > 0x7FFFFFFFu) {
        status[i] = JPEG_CORRUPT;
        continue;
      }
      std::vector<int> remap(script.tabs.size());
      for (size_t t = 0; t < script.tabs.size(); ++t) {
        auto it = seen_tabs.find(script.tab_keys[t]);
        if (it == seen_tabs.end()) {
          it = seen_tabs.emplace(script.tab_keys[t], (int)out->tabs.size()).first;
          out->tabs.push_back(script.tabs[t]);
        }
        remap[t] = it->second;
      }
      d.gpu = 3;
      d.scan_first = (int32_t)out->scans.size();
      d.nscans = (int32_t)script.scans.size();
      for (JpegProgScan s : script.scans) {
        for (int c = 0; c < 4; ++c)
          if (s.dc_tab[c] >= 0) s.dc_tab[c] = remap[(size_t)s.dc_tab[c]];
        if (s.ac_tab >= 0) s.ac_tab = remap[(size_t)s.ac_tab];
        out->scans.push_back(s);
      }
      jpeg_prog_frame_desc(h, &d);
      d.byte_off = out->byte_total;
      d.byte_len = (uint32_t)(len[i] - script.first_pos);
      d.byte_span = (uint32_t)round_up(d.byte_len, kJpegHuffBytePad);
      out->byte_total = round_up(d.byte_off + d.byte_span, kJpegHuffByteAlign);
      d.coef_base = out->coef_total;
      out->coef_total += (int64_t)h.total_coefs;
      continue;
    }
    RawSet& rs = rsv[0];
    rs = RawSet{};
    if (h.scan_pos > len[i] || len[i] - h.scan_pos > 0xFFFFFFF0u || !read_tables(data[i], len[i], h, &rs)) {
      status[i] = JPEG_CORRUPT;
      continue;
    }
    const std::string key = set_key(rs);
    auto it = seen.find(key);
    if (it == seen.end()) {
      JpegHuffSet s;
      bool ok = true;
      for (int t = 0; t < 4; ++t) ok = ok && build_tab(rs.t[t], &s.dc[t]) && build_tab(rs.t[4 + t], &s.ac[t]);
      if (!ok) {
        status[i] = JPEG_CORRUPT;
        continue;
      }
      it = seen.emplace(key, (int)out->sets.size()).first;
      out->sets.push_back(s);
    }
    d.gpu = 1;
    d.set_idx = it->second;
    d.byte_off = out->byte_total;
    d.byte_len = (uint32_t)(len[i] - h.scan_pos);
    if (par_sub_bits && h.restart_interval == 0 && h.ncomp != 4) {   // four components: the one-lane kernel
      const size_t k = destuff(data[i] + h.scan_pos, len[i] - h.scan_pos, nullptr, (size_t)-1);
      if (k < kJpegParMaxBits / 8u) {
        JpegParDesc& p = out->par[(size_t)i];
        d.gpu = 2;
        d.byte_len = (uint32_t)k;
        p.bit_len = (uint32_t)k * 8u;
        p.bpm = 0;
        for (int c = 0; c < h.ncomp; ++c) p.bpm += h.at(c).h * h.at(c).v;
        p.total_blocks = (uint32_t)h.mcux * (uint32_t)h.mcuy * (uint32_t)p.bpm;
        p.scan_pos = h.scan_pos;
        p.scratch_off = out->scratch_total;
        out->scratch_total += (int64_t)kJpegParStateWords * jpeg_par_nsub(p.bit_len, par_sub_bits);
      }
    }
    d.byte_span = (uint32_t)round_up(d.byte_len, kJpegHuffBytePad);
    out->byte_total = round_up(d.byte_off + d.byte_span, kJpegHuffByteAlign);
    d.coef_base = out->coef_total;
    d.total_coefs = h.total_coefs;
    out->coef_total += (int64_t)h.total_coefs;
    d.ncomp = h.ncomp;
    d.mcux = h.mcux;
    d.mcuy = h.mcuy;
    d.restart_interval = h.restart_interval;
    for (int c = 0; c < h.ncomp; ++c) {
      d.h[c] = h.at(c).h;
      d.v[c] = h.at(c).v;
      d.bw[c] = h.at(c).bw;
      d.bh[c] = h.at(c).bh;
      d.coef_off[c] = h.at(c).coef_off;
      d.td[c] = rs.td[c];
      d.ta[c] = rs.ta[c];
    }
    if (opt.restart_intervals && d.gpu == 1 && h.restart_interval > 0 && h.mcux >= 1 && h.mcuy >= 1 && h.ncomp != 4) {
      // one item per interval: the byte after each in-sequence RSTn, found by the reader's byte rules
      const int64_t ri = h.restart_interval;
      const int64_t need = ((int64_t)h.mcux * h.mcuy + ri - 1) / ri - 1;
      const uint8_t* s = data[i] + h.scan_pos;
      const size_t m = len[i] - h.scan_pos;
      begins.clear();
      size_t p = 0;
      while ((int64_t)begins.size() < need && p + 1 < m) {
        if (s[p] != 0xFFu) {
          ++p;
        } else if (s[p + 1] == 0xFFu) {
          ++p;                          // fill byte: look again from the next FF
        } else if (s[p + 1] == 0x00u) {
          p += 2;
        } else if (s[p + 1] == 0xD0u + (begins.size() & 7u)) {
          p += 2;
          begins.push_back((uint32_t)p);
        } else {
          break;                        // another marker, or an RSTn out of sequence
        }
      }
      // a marker with nothing behind it starts no interval: left to the one-lane kernel like a missing one
      const bool found = (int64_t)begins.size() == need && d.byte_len > 0 && (begins.empty() || begins.back() < d.byte_len);
      if (found && (int64_t)out->rst_items.size() + need + 1 < 0x7FFFFFFFll) {
        d.gpu = 4;
        for (int64_t k = 0; k <= need; ++k)
          out->rst_items.push_back(JpegRstItem{(int32_t)i, k ? begins[(size_t)k - 1] : 0u, (int32_t)(k * ri), (int32_t)k});
      }
    }
  }
}

void jpeg_huff_copy_bytes(const JpegHuffBatch& b, const uint8_t* const* data, const size_t* len, uint8_t* dst) {
  int64_t at = 0;
  for (size_t i = 0; i < b.desc.size(); ++i) {
    const JpegHuffDesc& d = b.desc[i];
    if (!d.gpu) continue;
    if (d.byte_off > at) std::memset(dst + at, 0, (size_t)(d.byte_off - at));
    if (d.gpu == 2) {
      // the span was sized by the same walk over the same bytes
      if (d.byte_span) std::memset(dst + d.byte_off, 0, d.byte_span);
      const size_t scan = b.par[i].scan_pos < len[i] ? b.par[i].scan_pos : len[i];
      if (d.byte_len) destuff(data[i] + scan, len[i] - scan, dst + d.byte_off, d.byte_len);
      at = d.byte_off + d.byte_span;
      continue;
    }
    if (d.byte_len) std::memcpy(dst + d.byte_off, data[i] + (len[i] - d.byte_len), d.byte_len);
    at = d.byte_off + d.byte_len;
  }
  if (b.byte_total > at) std::memset(dst + at, 0, (size_t)(b.byte_total - at));
}

namespace {

const char* check_all(const JpegHuffDesc* desc, const JpegParDesc* par, int n, int64_t byte_cap, int64_t nsets,
                      int64_t coef_cap, int64_t scratch_cap, uint32_t sub_bits, const JpegOptions& opt) {
  int64_t byte_at = 0, coef_at = 0;       // spans ascend with the entries: none may start before its predecessor ends
  int64_t scratch_at = 0;
  if (par != nullptr && (sub_bits < 32u || sub_bits > kJpegParMaxSubBits || sub_bits % 32u != 0)) return "sub-stream size";
  for (int i = 0; i < n; ++i) {
    const JpegHuffDesc& d = desc[i];
    if (!d.gpu) continue;
    if (d.gpu != 1 && !(d.gpu == 2 && par != nullptr) && !(d.gpu == 3 && opt.native_progressive) &&
        !(d.gpu == 4 && opt.restart_intervals))
      return "gpu flag";
    if (d.byte_off < byte_at || d.byte_off % kJpegHuffByteAlign != 0 || d.byte_len > d.byte_span ||
        d.byte_span % kJpegHuffBytePad != 0 || d.byte_off + (int64_t)d.byte_span > byte_cap)
      return "byte span outside the byte buffer";
    byte_at = d.byte_off + (int64_t)d.byte_span;
    if (d.gpu != 3 && (d.set_idx < 0 || d.set_idx >= nsets)) return "table set index";
    if (d.coef_base < coef_at || d.coef_base % 64 != 0 || d.coef_base + (int64_t)d.total_coefs > coef_cap)
      return "coefficient span outside the coefficient buffer";
    coef_at = d.coef_base + (int64_t)d.total_coefs;
    if ((d.ncomp != 1 && d.ncomp != 3 && d.ncomp != 4) || d.mcux < 1 || d.mcuy < 1 || d.mcux > kJpegMaxDim / 8 + 1 ||
        d.mcuy > kJpegMaxDim / 8 + 1 || d.restart_interval < 0 || d.restart_interval > 65535)
      return "frame";
    int64_t co = 0;
    for (int c = 0; c < d.ncomp; ++c) {
      if (d.h[c] < 1 || d.h[c] > 4 || d.v[c] < 1 || d.v[c] > 4 || d.bw[c] != d.mcux * d.h[c] ||
          d.bh[c] != d.mcuy * d.v[c] || (int64_t)d.coef_off[c] != co || d.td[c] < 0 || d.td[c] > 3 || d.ta[c] < 0 ||
          d.ta[c] > 3)
        return "component layout";
      co += (int64_t)d.bw[c] * d.bh[c] * 64;
    }
    if (co != (int64_t)d.total_coefs) return "coefficient count";
    if (!opt.native_sampling && d.ncomp == 3 && d.h[1] == 1 && d.v[1] == 1 && d.h[2] == 1 && d.v[2] == 1 &&
        ((d.h[0] == 1 && d.v[0] == 2) || (d.h[0] == 4 && d.v[0] == 1)))
      return "sampling layout of a batch planned without native_sampling";
    if (d.ncomp == 4) {
      if (!opt.native_colorspace) return "four components in a batch planned without native_colorspace";
      if (d.gpu == 2 || d.gpu == 4) return "four components outside the one-lane and progressive kernels";
      for (int c = 0; c < 4; ++c)
        if (d.h[c] != 1 || d.v[c] != 1) return "four components not all 1x1";
    }
    if (d.gpu == 4 && d.restart_interval < 1) return "restart interval";
    if (d.gpu == 2) {
      const JpegParDesc& p = par[i];
      int bpm = 0;
      for (int c = 0; c < d.ncomp; ++c) bpm += d.h[c] * d.v[c];
      if (d.restart_interval != 0 || d.byte_len >= kJpegParMaxBits / 8u || p.bit_len != d.byte_len * 8u ||
          p.bpm != bpm || bpm > 63 || (int64_t)p.total_blocks != (int64_t)d.mcux * d.mcuy * bpm)
        return "sub-stream descriptor";
      const int64_t words = (int64_t)kJpegParStateWords * jpeg_par_nsub(p.bit_len, sub_bits);
      if (p.scratch_off < scratch_at || p.scratch_off + words > scratch_cap) return "scratch span outside the scratch buffer";
      scratch_at = p.scratch_off + words;
    }
  }
  return nullptr;
}

}  // namespace

const char* jpeg_huff_check(const JpegHuffDesc* desc, int n, int64_t byte_cap, int64_t nsets, int64_t coef_cap,
                            const JpegOptions& opt) {
  return check_all(desc, nullptr, n, byte_cap, nsets, coef_cap, 0, 0, opt);
}

const char* jpeg_huff_par_check(const JpegHuffDesc* desc, const JpegParDesc* par, int n, int64_t byte_cap,
                                int64_t nsets, int64_t coef_cap, int64_t scratch_cap, uint32_t sub_bits,
                                const JpegOptions& opt) {
  if (par == nullptr) return "no sub-stream descriptors";
  return check_all(desc, par, n, byte_cap, nsets, coef_cap, scratch_cap, sub_bits, opt);
}

const char* jpeg_huff_prog_check(const JpegHuffDesc* desc, int n, const JpegProgScan* scans, int64_t nscans,
                                 int64_t ntabs) {
  int64_t scan_at = 0;                    // ranges ascend with the entries
  for (int i = 0; i < n; ++i) {
    const JpegHuffDesc& d = desc[i];
    if (d.gpu != 3) continue;
    if (scans == nullptr || d.nscans < 1 || d.nscans > kJpegProgMaxScans || (int64_t)d.scan_first < scan_at ||
        (int64_t)d.scan_first + d.nscans > nscans)
      return "scan range outside the scan buffer";
    scan_at = (int64_t)d.scan_first + d.nscans;
    if (d.ncomp != 1 && d.ncomp != 3 && d.ncomp != 4) return "frame";
    for (int c = 0; c < d.ncomp; ++c)
      if (d.gw[c] < 1 || d.gh[c] < 1 || d.gw[c] > d.bw[c] || d.gh[c] > d.bh[c] || d.gw[c] <= d.bw[c] - d.h[c] ||
          d.gh[c] <= d.bh[c] - d.v[c])
        return "component grid";
    uint32_t off_at = 0;                  // scans follow each other in the span
    for (int k = 0; k < d.nscans; ++k) {
      const JpegProgScan& s = scans[d.scan_first + k];
      if (s.byte_off < off_at || s.byte_off > d.byte_len) return "scan offset outside the byte span";
      off_at = s.byte_off;
      if (s.ncomp < 1 || s.ncomp > d.ncomp) return "scan components";
      for (int q = 0; q < s.ncomp; ++q)
        if (s.comp[q] < 0 || s.comp[q] >= d.ncomp || (q > 0 && s.comp[q] <= s.comp[q - 1])) return "scan components";
      if (s.ss < 0 || s.se > 63 || s.ss > s.se || s.al < 0 || s.al > 13 || (s.ah != 0 && s.ah != s.al + 1) ||
          (s.ss == 0 ? s.se != 0 : s.ncomp != 1) || s.restart_interval < 0 || s.restart_interval > 65535)
        return "scan parameters";
      for (int q = 0; q < s.ncomp; ++q)
        if (s.ss == 0 && s.ah == 0 && (s.dc_tab[q] < 0 || s.dc_tab[q] >= ntabs)) return "DC table index";
      if (s.ss != 0 && (s.ac_tab < 0 || s.ac_tab >= ntabs)) return "AC table index";
    }
  }
  return nullptr;
}

const char* jpeg_huff_rst_check(const JpegHuffDesc* desc, int n, const JpegRstItem* items, int64_t nitems) {
  if (nitems < 0 || nitems >= 0x7FFFFFFFll || (nitems > 0 && items == nullptr)) return "item count";
  int64_t at = 0;                         // items follow the entries
  for (int i = 0; i < n; ++i) {
    const JpegHuffDesc& d = desc[i];
    if (d.gpu != 4) continue;
    if (d.restart_interval < 1 || d.mcux < 1 || d.mcuy < 1) return "restart interval";
    const int64_t ri = d.restart_interval, mcus = (int64_t)d.mcux * d.mcuy;
    const int64_t count = (mcus + ri - 1) / ri;
    if (at + count > nitems) return "items of an entry missing";
    uint32_t begin_at = 0;
    for (int64_t k = 0; k < count; ++k) {
      const JpegRstItem& it = items[at + k];
      if (it.entry != i || (int64_t)it.index != k) return "items not contiguous and ascending";
      if ((int64_t)it.mcu_first != k * ri || (int64_t)it.mcu_first >= mcus) return "item's first MCU";
      if (it.byte_begin >= d.byte_len || it.byte_begin < begin_at) return "item's first byte outside the byte span";
      begin_at = it.byte_begin;
    }
    at += count;
  }
  if (at != nitems) return "item of an entry that is not a restart-interval entry";
  return nullptr;
}

}  // namespace idunno
