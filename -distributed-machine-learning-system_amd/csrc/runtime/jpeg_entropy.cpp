// Baseline JPEG marker parser and Huffman decoder (see jpeg_entropy.h).
//
// Every read of the input goes through a bounds check against the span's end
// and every write of a coefficient through an index check (k <= 63 inside a
// block that the header-derived layout places inside the output span), so
// arbitrary bytes give a status, never an out-of-range access.
//
// What JpegOptions admits costs no second path: the parser also walks a progressive file's
// scans up to EOI into a scan script, which jpeg_decode hands to the shared scan core of
// ../jpeg_huff_prog.h (baseline files take the same path as without it); the decode loops take
// every h, v in 1..4 and every ncomp from the header, so modes 3 and 4 and four components run
// through them unchanged.
#include "jpeg_entropy.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

namespace idunno {

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;

struct Huff {
  bool defined = false;
  int nvals = 0;
  uint8_t vals[256];
  uint16_t look[1 << kLookBits];   // (length << 8) | symbol for codes of <= kLookBits bits, else 0
  int32_t maxcode[17];             // largest code of each length, -1: none
  int32_t mincode[17];
  int32_t valptr[17];
};

// counts[1..16] then the symbols; returns bytes consumed or -1
int build_huff(const uint8_t* seg, size_t slen, Huff* h) {
  if (slen < 16) return -1;
  int counts[17];
  int total = 0;
  for (int l = 1; l <= 16; ++l) {
    counts[l] = seg[l - 1];
    total += counts[l];
  }
  if (total > 256 || (size_t)(16 + total) > slen) return -1;
  std::memcpy(h->vals, seg + 16, (size_t)total);
  h->nvals = total;
  std::memset(h->look, 0, sizeof(h->look));
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    if (code + counts[l] > (1 << l)) return -1;        // more codes than the length has room for
    h->valptr[l] = k;
    h->mincode[l] = code;
    h->maxcode[l] = counts[l] ? code + counts[l] - 1 : -1;
    if (l <= kLookBits) {
      for (int i = 0; i < counts[l]; ++i) {
        const int first = (code + i) << (kLookBits - l);
        for (int j = 0; j < (1 << (kLookBits - l)); ++j)
          h->look[first + j] = (uint16_t)((l << 8) | h->vals[k + i]);
      }
    }
    k += counts[l];
    code = (code + counts[l]) << 1;
  }
  h->defined = true;
  return 16 + total;
}

struct Tables {
  bool qdef[4] = {false, false, false, false};
  uint16_t q[4][64];
  Huff dc[4], ac[4];
};

struct Scan {
  int td[4], ta[4];
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// The DHT payloads of a progressive file's table slots (dc 0..3, ac 0..3), kept
// because each SOS of the scan script latches the tables in effect there.
struct RawTabs {
  std::string key[8];     // class byte, 16 counts, the symbols; empty: undefined
};

// the table of a DHT payload build_huff has accepted, in the core's form
void build_core_tab(const std::string& key, JpegHuffTab* t) {
  const uint8_t* counts = reinterpret_cast<const uint8_t*>(key.data()) + 1;
  const uint8_t* vals = counts + 16;
  std::memset(t, 0, sizeof(*t));
  t->maxcode[0] = -1;
  t->nvals = (int32_t)key.size() - 17;
  std::memcpy(t->vals, vals, (size_t)t->nvals);
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = counts[l - 1];
    t->valptr[l] = k;
    t->mincode[l] = code;
    t->maxcode[l] = cnt ? code + cnt - 1 : -1;
    if (l <= kJpegHuffLookBits) {
      const int rep = 1 << (kJpegHuffLookBits - l);
      for (int i = 0; i < cnt; ++i)
        for (int j = 0; j < rep; ++j) t->look[(code + i) * rep + j] = (uint16_t)((l << 8) | vals[k + i]);
    }
    k += cnt;
    code = (code + cnt) << 1;
  }
}

// index of the slot's table in script->tabs, added on first use
int script_tab(const RawTabs& raw, int slot, JpegProgScript* script) {
  const std::string& key = raw.key[slot];
  for (size_t i = 0; i < script->tab_keys.size(); ++i)
    if (script->tab_keys[i] == key) return (int)i;
  script->tab_keys.push_back(key);
  script->tabs.emplace_back();
  build_core_tab(key, &script->tabs.back());
  return (int)script->tabs.size() - 1;
}

// opt: see JpegOptions; script, when given, receives the scans of a progressive file
int parse(const uint8_t* data, size_t n, JpegHeader* hdr, Tables* tb, Scan* sc, const JpegOptions& opt,
          JpegProgScript* script = nullptr) {
  const bool native = opt.native_progressive, sampling = opt.native_sampling, color = opt.native_colorspace;
  if (data == nullptr || n == 0) return JPEG_EMPTY;
  if (n < 2 || data[0] != 0xFF || data[1] != 0xD8) return JPEG_NOT_JPEG;
  std::memset(hdr, 0, sizeof(*hdr));
  if (script != nullptr) *script = JpegProgScript{};
  bool have_sof = false;
  int comp_id[4] = {0, 0, 0, 0};
  bool latched[4] = {false, false, false, false};
  bool jfif = false, adobe = false;
  int adobe_transform = 0;
  // libjpeg's rules, applied at the first SOS (every APPn in front of it has been seen): false: refused
  auto classify = [&]() {
    hdr->colorspace = 0;
    if (!color) return true;
    if (hdr->ncomp == 3) {
      if (jfif) return true;
      if (adobe) hdr->colorspace = adobe_transform == 0 ? 1 : 0;
      else if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') hdr->colorspace = 1;
    } else if (hdr->ncomp == 4) {
      if (!adobe || adobe_transform == 0) hdr->colorspace = 2;
      else if (adobe_transform == 2) hdr->colorspace = 3;
      else return false;
    }
    return true;
  };
  std::vector<RawTabs> rawv(native ? 1 : 0);            // off the stack
  size_t pos = 2;
  for (;;) {
    if (pos + 2 > n || data[pos] != 0xFF) return JPEG_CORRUPT;
    while (pos < n && data[pos] == 0xFF) ++pos;         // fill bytes
    if (pos >= n) return JPEG_CORRUPT;
    const int m = data[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
    if (m == 0xD9 && hdr->progressive && hdr->nscans > 0) return JPEG_OK;   // the walk's end
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return JPEG_CORRUPT;
    if (pos + 2 > n) return JPEG_CORRUPT;
    const int L = be16(data + pos);
    if (L < 2 || pos + (size_t)L > n) return JPEG_CORRUPT;
    const uint8_t* seg = data + pos + 2;
    const size_t slen = (size_t)L - 2;
    pos += (size_t)L;
    switch (m) {
      case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8:
        return JPEG_UNSUPPORTED_SOF;
      case 0xC9: case 0xCA: case 0xCB: case 0xCC: case 0xCD: case 0xCE: case 0xCF:
        return JPEG_UNSUPPORTED_ARITHMETIC;
      case 0xC2:
        if (!native) return JPEG_UNSUPPORTED_PROGRESSIVE;
        [[fallthrough]];                                 // the same frame header
      case 0xC0: case 0xC1: {
        if (have_sof || slen < 6) return JPEG_CORRUPT;
        if (seg[0] != 8) return JPEG_UNSUPPORTED_PRECISION;
        const int H = be16(seg + 1), W = be16(seg + 3), nf = seg[5];
        if (nf != 1 && nf != 3 && !(color && nf == 4)) return nf == 0 ? JPEG_CORRUPT : JPEG_UNSUPPORTED_COMPONENTS;
        if (slen != (size_t)(6 + 3 * nf) || W == 0 || H == 0) return JPEG_CORRUPT;
        if (W > kJpegMaxDim || H > kJpegMaxDim) return JPEG_UNSUPPORTED_SIZE;
        hdr->W = W;
        hdr->H = H;
        hdr->ncomp = nf;
        for (int c = 0; c < nf; ++c) {
          comp_id[c] = seg[6 + 3 * c];
          const int hv = seg[7 + 3 * c], tq = seg[8 + 3 * c];
          const int h = hv >> 4, v = hv & 15;
          if (h < 1 || h > 4 || v < 1 || v > 4 || tq > 3) return JPEG_CORRUPT;
          hdr->at(c).h = nf == 1 ? 1 : h;             // one component: never interleaved
          hdr->at(c).v = nf == 1 ? 1 : v;
          hdr->at(c).qidx = tq;
        }
        if (nf == 3) {
          const JpegComp* cp = hdr->comp;
          if (cp[1].h != cp[2].h || cp[1].v != cp[2].v) return JPEG_UNSUPPORTED_SAMPLING;
          if (cp[0].h == cp[1].h && cp[0].v == cp[1].v) hdr->mode = 0;
          else if (cp[1].h == 1 && cp[1].v == 1 && cp[0].h == 2 && cp[0].v == 1) hdr->mode = 1;
          else if (cp[1].h == 1 && cp[1].v == 1 && cp[0].h == 2 && cp[0].v == 2) hdr->mode = 2;
          else if (sampling && cp[1].h == 1 && cp[1].v == 1 && cp[0].h == 1 && cp[0].v == 2) hdr->mode = 3;
          else if (sampling && cp[1].h == 1 && cp[1].v == 1 && cp[0].h == 4 && cp[0].v == 1) hdr->mode = 4;
          else return JPEG_UNSUPPORTED_SAMPLING;
        }
        if (nf == 4)                                     // CMYK / YCCK: as libjpeg writes them, every component 1x1
          for (int c = 0; c < 4; ++c)
            if (hdr->at(c).h != 1 || hdr->at(c).v != 1) return JPEG_UNSUPPORTED_SAMPLING;
        hdr->hmax = hdr->comp[0].h;
        hdr->vmax = hdr->comp[0].v;
        hdr->mcux = (W + 8 * hdr->hmax - 1) / (8 * hdr->hmax);
        hdr->mcuy = (H + 8 * hdr->vmax - 1) / (8 * hdr->vmax);
        uint32_t off = 0;
        for (int c = 0; c < nf; ++c) {
          JpegComp& cp = hdr->at(c);
          cp.bw = hdr->mcux * cp.h;
          cp.bh = hdr->mcuy * cp.v;
          cp.coef_off = off;
          off += (uint32_t)cp.bw * (uint32_t)cp.bh * 64u;
        }
        hdr->total_coefs = off;
        hdr->progressive = m == 0xC2;
        have_sof = true;
        break;
      }
      case 0xDB: {
        size_t p = 0;
        while (p < slen) {
          const int pq = seg[p] >> 4, tq = seg[p] & 15;
          if (pq == 1) return JPEG_UNSUPPORTED_QUANT16;
          if (pq != 0 || tq > 3 || p + 65 > slen) return JPEG_CORRUPT;
          for (int k = 0; k < 64; ++k) tb->q[tq][kZigzag[k]] = seg[p + 1 + k];
          tb->qdef[tq] = true;
          p += 65;
        }
        break;
      }
      case 0xC4: {
        size_t p = 0;
        while (p < slen) {
          const int tc = seg[p] >> 4, th = seg[p] & 15;
          if (tc > 1 || th > 3) return JPEG_CORRUPT;
          const int used = build_huff(seg + p + 1, slen - p - 1, tc ? &tb->ac[th] : &tb->dc[th]);
          if (used < 0) return JPEG_CORRUPT;
          if (native) {
            std::string& key = rawv[0].key[4 * tc + th];
            key.assign(reinterpret_cast<const char*>(seg + p), 1 + (size_t)used);
            key[0] = (char)tc;                           // the slot does not tell tables apart
          }
          p += 1 + (size_t)used;
        }
        break;
      }
      case 0xDD:
        if (slen != 2) return JPEG_CORRUPT;
        hdr->restart_interval = be16(seg);
        break;
      case 0xDA: {
        if (!have_sof || slen < 1) return JPEG_CORRUPT;
        const int ns = seg[0];
        if (ns < 1 || ns > 4 || slen != (size_t)(4 + 2 * ns)) return JPEG_CORRUPT;
        if (hdr->progressive) {
          if (hdr->nscans >= kJpegProgMaxScans) return JPEG_UNSUPPORTED_MULTISCAN;
          if (ns > hdr->ncomp) return JPEG_CORRUPT;
          const RawTabs& raw = rawv[0];
          JpegProgScan s;
          std::memset(&s, 0, sizeof(s));
          s.ncomp = ns;
          s.ac_tab = s.dc_tab[0] = s.dc_tab[1] = s.dc_tab[2] = s.dc_tab[3] = -1;
          const uint8_t* t = seg + 1 + 2 * ns;
          s.ss = t[0];
          s.se = t[1];
          s.ah = t[2] >> 4;
          s.al = t[2] & 15;
          if (s.se > 63 || s.ss > s.se || s.al > 13 || (s.ah != 0 && s.ah != s.al + 1)) return JPEG_CORRUPT;
          if (s.ss == 0 ? s.se != 0 : ns != 1) return JPEG_CORRUPT;
          int td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0};
          for (int c = 0; c < ns; ++c) {
            int ci = -1;
            for (int f = 0; f < hdr->ncomp; ++f)
              if (comp_id[f] == seg[1 + 2 * c]) ci = f;
            if (ci < 0 || (c > 0 && ci <= s.comp[c - 1])) return JPEG_CORRUPT;   // frame order, none twice
            s.comp[c] = ci;
            td[c] = seg[2 + 2 * c] >> 4;
            ta[c] = seg[2 + 2 * c] & 15;
            if (td[c] > 3 || ta[c] > 3) return JPEG_CORRUPT;
            // only the table the scan decodes with has to exist: DC first scans a DC table, AC scans an AC table
            if (s.ss == 0 ? (s.ah == 0 && raw.key[td[c]].empty()) : raw.key[4 + ta[c]].empty()) return JPEG_CORRUPT;
            if (!latched[ci]) {
              if (!tb->qdef[hdr->at(ci).qidx]) return JPEG_CORRUPT;
              std::memcpy(hdr->at(ci).q, tb->q[hdr->at(ci).qidx], sizeof(hdr->at(ci).q));
              latched[ci] = true;
            }
          }
          if (hdr->nscans == 0 && !classify()) return JPEG_UNSUPPORTED_COMPONENTS;
          if (hdr->nscans == 0) hdr->scan_pos = (uint32_t)pos;
          if (script != nullptr) {
            if (hdr->nscans == 0) script->first_pos = (uint32_t)pos;
            s.byte_off = (uint32_t)(pos - script->first_pos);
            s.restart_interval = hdr->restart_interval;
            for (int c = 0; c < ns; ++c)
              if (s.ss == 0 && s.ah == 0) s.dc_tab[c] = script_tab(raw, td[c], script);
            if (s.ss != 0) s.ac_tab = script_tab(raw, 4 + ta[0], script);
            script->scans.push_back(s);
          }
          ++hdr->nscans;
          // over the entropy-coded data to the next marker that is not RSTn; none: no EOI
          while (pos + 1 < n && !(data[pos] == 0xFF && data[pos + 1] != 0x00 && data[pos + 1] != 0xFF &&
                                  !(data[pos + 1] >= 0xD0 && data[pos + 1] <= 0xD7)))
            ++pos;
          if (pos + 1 >= n) return JPEG_CORRUPT;
          break;
        }
        if (ns != hdr->ncomp) return JPEG_UNSUPPORTED_MULTISCAN;
        for (int c = 0; c < ns; ++c) {
          if (seg[1 + 2 * c] != comp_id[c]) return JPEG_CORRUPT;
          const int t = seg[2 + 2 * c];
          sc->td[c] = t >> 4;
          sc->ta[c] = t & 15;
          if (sc->td[c] > 3 || sc->ta[c] > 3) return JPEG_CORRUPT;
          if (!tb->dc[sc->td[c]].defined || !tb->ac[sc->ta[c]].defined) return JPEG_CORRUPT;
          if (!tb->qdef[hdr->at(c).qidx]) return JPEG_CORRUPT;
          std::memcpy(hdr->at(c).q, tb->q[hdr->at(c).qidx], sizeof(hdr->at(c).q));
        }
        const uint8_t* t = seg + 1 + 2 * ns;
        if (t[0] != 0 || t[1] != 63 || t[2] != 0) return JPEG_CORRUPT;
        if (!classify()) return JPEG_UNSUPPORTED_COMPONENTS;
        hdr->scan_pos = (uint32_t)pos;
        hdr->nscans = 1;
        return JPEG_OK;
      }
      case 0xE0:                                         // APP0: "JFIF\0" and at least the 14 bytes libjpeg asks for
        if (slen >= 14 && std::memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
        break;
      case 0xEE:                                         // APP14: "Adobe", version, flags0, flags1, transform
        if (slen >= 12 && std::memcmp(seg, "Adobe", 5) == 0) {
          adobe = true;
          adobe_transform = seg[11];
        }
        break;
      default:                                           // other APPn, COM and anything else with a length
        break;
    }
  }
}

// MSB-first bit reader over the entropy-coded segment: removes byte stuffing,
// stops at a marker (feeding zero bits the decoder must not consume).
struct BitReader {
  const uint8_t* data;
  size_t p, end;
  uint64_t acc = 0;
  int nbits = 0;       // bits in acc
  int pad = 0;         // of which zero bits made up past a marker / the end (always the lowest)
  bool stopped = false;
  bool overrun = false;

  void fill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (!stopped) {
        if (p >= end) {
          stopped = true;
        } else if (data[p] != 0xFF) {
          b = data[p++];
        } else if (p + 1 >= end) {
          stopped = true;
        } else if (data[p + 1] == 0x00) {
          b = 0xFF;
          p += 2;
        } else if (data[p + 1] == 0xFF) {
          ++p;                                           // fill byte
          continue;
        } else {
          stopped = true;                                // a marker: stay on its 0xFF
        }
      }
      if (stopped) pad += 8;
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  inline void ensure() {
    if (nbits < 32) fill();
  }
  inline unsigned peek(int k) const { return (unsigned)(acc >> (nbits - k)) & ((1u << k) - 1u); }
  inline void skip(int k) {
    nbits -= k;
    if (nbits < pad) {
      overrun = true;
      pad = nbits;
    }
  }
  inline unsigned get(int k) {
    const unsigned v = peek(k);
    skip(k);
    return v;
  }
  // byte-align and consume RSTn; false: not there
  bool restart(int idx) {
    if (nbits - pad >= 8) return false;                  // whole data bytes in front of the marker
    acc = 0;
    nbits = pad = 0;
    stopped = false;
    if (p + 2 > end || data[p] != 0xFF) return false;
    while (p < end && data[p] == 0xFF) ++p;
    if (p >= end || data[p] != 0xD0 + (idx & 7)) return false;
    ++p;
    return true;
  }
};

// a Huffman symbol, or -1 on a code the table does not hold
inline int decode_sym(BitReader& br, const Huff& h) {
  br.ensure();
  const unsigned e = h.look[br.peek(kLookBits)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const unsigned c16 = br.peek(16);
  for (int l = kLookBits + 1; l <= 16; ++l) {
    const int32_t c = (int32_t)(c16 >> (16 - l));
    if (h.maxcode[l] >= 0 && c <= h.maxcode[l] && c >= h.mincode[l]) {
      const int idx = h.valptr[l] + (c - h.mincode[l]);
      if (idx >= h.nvals) return -1;
      br.skip(l);
      return h.vals[idx];
    }
  }
  return -1;
}

inline int receive_extend(BitReader& br, int s) {
  br.ensure();
  const int v = (int)br.get(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// one 8x8 block into blk[64] (zeroed by the caller); false on corruption
bool decode_block(BitReader& br, const Huff& dc, const Huff& ac, int* pred, int16_t* blk) {
  int s = decode_sym(br, dc);
  if (s < 0 || s > 15) return false;
  if (s) *pred += receive_extend(br, s);
  if (*pred < -32768 || *pred > 32767) return false;
  blk[0] = (int16_t)*pred;
  int k = 1;
  while (k < 64) {
    const int rs = decode_sym(br, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                                // EOB
      k += 16;                                           // ZRL
      if (k > 64) return false;
      continue;
    }
    k += r;
    if (k > 63) return false;
    blk[kZigzag[k]] = (int16_t)receive_extend(br, s);
    ++k;
  }
  return !br.overrun;
}

}  // namespace

const char* jpeg_status_name(int status) {
  static const char* const names[JPEG_STATUS_COUNT] = {
      "ok", "empty", "not_jpeg", "corrupt", "progressive", "arithmetic", "precision", "components",
      "quant16", "sampling", "size", "multiscan", "sof", "buffer_too_small"};
  return status >= 0 && status < JPEG_STATUS_COUNT ? names[status] : "unknown";
}

int jpeg_parse_header(const uint8_t* data, size_t n, JpegHeader* hdr, const JpegOptions& opt, JpegProgScript* script) {
  std::vector<Tables> tb(1);                             // ~9 KB: off the stack
  Scan sc;
  return parse(data, n, hdr, &tb[0], &sc, opt, script);
}

void jpeg_prog_frame_desc(const JpegHeader& h, JpegHuffDesc* d) {
  d->total_coefs = h.total_coefs;
  d->ncomp = h.ncomp;
  d->mcux = h.mcux;
  d->mcuy = h.mcuy;
  for (int c = 0; c < h.ncomp && c < 4; ++c) {
    const JpegComp& cp = h.at(c);
    d->h[c] = cp.h;
    d->v[c] = cp.v;
    d->bw[c] = cp.bw;
    d->bh[c] = cp.bh;
    d->coef_off[c] = cp.coef_off;
    d->gw[c] = ((h.W * cp.h + h.hmax - 1) / h.hmax + 7) / 8;
    d->gh[c] = ((h.H * cp.v + h.vmax - 1) / h.vmax + 7) / 8;
  }
}

namespace {

// a progressive file parse() accepted, with the shared core: the scans' bytes (first scan's
// data to the end of the file) go to a word-aligned, padded copy, which is what Bits reads
int decode_progressive(const uint8_t* data, size_t n, const JpegHeader& hdr, const JpegProgScript& script,
                       int16_t* out) {
  if (script.first_pos > n || n - script.first_pos > 0xFFFFFFF0u) return JPEG_CORRUPT;
  JpegHuffDesc d;
  std::memset(&d, 0, sizeof(d));
  jpeg_prog_frame_desc(hdr, &d);
  d.byte_len = (uint32_t)(n - script.first_pos);
  d.byte_span = (d.byte_len + (uint32_t)kJpegHuffBytePad - 1u) / (uint32_t)kJpegHuffBytePad * (uint32_t)kJpegHuffBytePad;
  d.scan_first = 0;
  d.nscans = (int32_t)script.scans.size();
  std::vector<uint32_t> words(d.byte_span / 4 + 1, 0u);
  std::memcpy(words.data(), data + script.first_pos, d.byte_len);
  return jpeg_prog_decode_image(d, script.scans.data(), (long long)script.scans.size(), words.data(),
                                script.tabs.data(), (int32_t)script.tabs.size(), out);
}

}  // namespace

int jpeg_decode(const uint8_t* data, size_t n, JpegHeader* hdr, int16_t* out, size_t out_cap, const JpegOptions& opt) {
  std::vector<Tables> tbv(1);
  Tables& tb = tbv[0];
  Scan sc;
  JpegProgScript script;
  const int st = parse(data, n, hdr, &tb, &sc, opt, opt.native_progressive ? &script : nullptr);
  if (st != JPEG_OK) return st;
  if (out == nullptr || (size_t)hdr->total_coefs > out_cap) return JPEG_BUFFER_TOO_SMALL;
  std::memset(out, 0, (size_t)hdr->total_coefs * sizeof(int16_t));
  if (hdr->progressive) return decode_progressive(data, n, *hdr, script, out);
  BitReader br;
  br.data = data;
  br.p = hdr->scan_pos;
  br.end = n;
  int pred[4] = {0, 0, 0, 0};
  const int ri = hdr->restart_interval;
  int left = ri, rst = 0;
  for (int my = 0; my < hdr->mcuy; ++my) {
    for (int mx = 0; mx < hdr->mcux; ++mx) {
      if (ri) {
        if (left == 0) {
          if (!br.restart(rst++)) return JPEG_CORRUPT;
          pred[0] = pred[1] = pred[2] = pred[3] = 0;
          left = ri;
        }
        --left;
      }
      for (int c = 0; c < hdr->ncomp; ++c) {
        const JpegComp& cp = hdr->at(c);
        for (int by = 0; by < cp.v; ++by) {
          for (int bx = 0; bx < cp.h; ++bx) {
            const size_t b = (size_t)(my * cp.v + by) * (size_t)cp.bw + (size_t)(mx * cp.h + bx);
            if (!decode_block(br, tb.dc[sc.td[c]], tb.ac[sc.ta[c]], &pred[c], out + cp.coef_off + b * 64))
              return JPEG_CORRUPT;
          }
        }
      }
    }
  }
  return JPEG_OK;
}

void jpeg_decode_batch(int n, const uint8_t* const* data, const size_t* len, JpegHeader* hdr,
                       int16_t* const* out, const size_t* out_cap, int* status, int nthreads, const JpegOptions& opt) {
  std::atomic<int> next{0};
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n) return;
      status[i] = data[i] == nullptr ? (int)JPEG_EMPTY : jpeg_decode(data[i], len[i], &hdr[i], out[i], out_cap[i], opt);
    }
  };
  const int nt = std::max(1, std::min(nthreads, n));
  std::vector<std::thread> th;
  th.reserve((size_t)nt - 1);
  for (int i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

}  // namespace idunno
