// Host stage of the JPEG ingest: marker parser + sequential Huffman decoder (ITU-T T.81 baseline / extended sequential, 8-bit).
// The input is untrusted: every read goes through a bounds check, every table index, code, run and position is validated, and a
// stream that is short or wrong ends in a status -- never in libjpeg's "pad with zeros and warn".  No HIP in this file.
#include "jpeg_host.h"

#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

namespace wvn_jpeg {
namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;   // bits of the one-step Huffman lookup

struct Huff {
  bool defined = false;
  uint8_t look_len[1 << kLook];   // 0: longer than kLook bits (or no such code)
  uint8_t look_sym[1 << kLook];
  int32_t maxcode[18];            // largest code of length l, -1 when none
  int32_t valoff[17];             // huffval index of the first code of length l minus that code
  uint8_t huffval[256];
  int nsym = 0;
};

struct Component {
  int id, h, v, tq, td, ta;
};

struct Header {
  int width = 0, height = 0, ncomp = 0, restart = 0;
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  Component comp[3];
  uint16_t qt[4][64];
  bool qt_defined[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  size_t scan = 0;   // first byte of the entropy-coded segment
};

int sampling_of(const Header& h) {
  if (h.ncomp == 1) return WVN_JPEG_GRAY;
  if (h.comp[1].h != 1 || h.comp[1].v != 1 || h.comp[2].h != 1 || h.comp[2].v != 1) return -1;
  const int H = h.comp[0].h, V = h.comp[0].v;
  if (H == 1 && V == 1) return WVN_JPEG_444;
  if (H == 2 && V == 1) return WVN_JPEG_422;
  if (H == 2 && V == 2) return WVN_JPEG_420;
  return -1;
}

int build_huff(Huff& t, const uint8_t* bits /* [16] */, const uint8_t* vals, int nvals, bool is_dc) {
  // canonical codes (T.81 annex C); the code space must not be oversubscribed
  memset(t.look_len, 0, sizeof(t.look_len));
  memset(t.look_sym, 0, sizeof(t.look_sym));
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    t.valoff[l] = k - code;
    if (n) {
      if (code + n > (1 << l)) return WVN_JPEG_BAD_TABLE;
      for (int i = 0; i < n; ++i, ++k, ++code) {
        if (k >= nvals) return WVN_JPEG_BAD_TABLE;
        if (is_dc && vals[k] > 15) return WVN_JPEG_BAD_TABLE;
        t.huffval[k] = vals[k];
        if (l <= kLook) {
          const int first = code << (kLook - l);
          for (int j = 0; j < (1 << (kLook - l)); ++j) {
            t.look_len[first + j] = (uint8_t)l;
            t.look_sym[first + j] = vals[k];
          }
        }
      }
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.nsym = k;
  t.defined = true;
  return WVN_JPEG_OK;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS.  On WVN_JPEG_OK h.scan is the first entropy-coded byte.  build_tables false: the geometry probe
// of a batch -- a DHT is checked for its lengths only and its codes are not built (the decode that follows does that and has the say).
int parse_header(const uint8_t* d, size_t n, Header& h, bool build_tables) {
  if (d == nullptr || n < 2) return WVN_JPEG_TRUNCATED;
  if (d[0] != 0xFF || d[1] != 0xD8) return WVN_JPEG_BAD_MARKER;
  size_t p = 2;
  for (;;) {
    if (p >= n) return WVN_JPEG_TRUNCATED;
    if (d[p] != 0xFF) return WVN_JPEG_BAD_MARKER;
    while (p < n && d[p] == 0xFF) ++p;   // fill bytes
    if (p >= n) return WVN_JPEG_TRUNCATED;
    const int m = d[p++];
    if (m == 0xD9) return WVN_JPEG_TRUNCATED;                                  // EOI before any scan
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return WVN_JPEG_BAD_MARKER;   // stand-alone markers have no place here
    if (p + 2 > n) return WVN_JPEG_TRUNCATED;
    const int len = be16(d + p);
    if (len < 2) return WVN_JPEG_BAD_MARKER;
    if (p + (size_t)len > n) return WVN_JPEG_TRUNCATED;
    const uint8_t* s = d + p + 2;
    const int sl = len - 2;
    p += (size_t)len;
    switch (m) {
      case 0xC0:
      case 0xC1: {
        if (h.have_sof) return WVN_JPEG_BAD_MARKER;
        if (sl < 6) return WVN_JPEG_BAD_MARKER;
        if (s[0] != 8) return WVN_JPEG_UNSUPPORTED;   // 12-bit samples
        h.height = be16(s + 1);
        h.width = be16(s + 3);
        const int nc = s[5];
        if (sl != 6 + 3 * nc) return WVN_JPEG_BAD_MARKER;
        if (nc != 1 && nc != 3) return WVN_JPEG_UNSUPPORTED;   // CMYK / YCCK / two components
        if (h.height == 0 || h.width == 0) return WVN_JPEG_UNSUPPORTED;   // (height 0: a DNL marker would define it)
        if (h.height > WVN_JPEG_MAX_DIM || h.width > WVN_JPEG_MAX_DIM) return WVN_JPEG_UNSUPPORTED;
        h.ncomp = nc;
        for (int c = 0; c < nc; ++c) {
          Component& k = h.comp[c];
          k.id = s[6 + 3 * c];
          k.h = s[7 + 3 * c] >> 4;
          k.v = s[7 + 3 * c] & 15;
          k.tq = s[8 + 3 * c];
          k.td = k.ta = -1;
          if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return WVN_JPEG_BAD_MARKER;
          if (k.tq > 3) return WVN_JPEG_BAD_TABLE;
          for (int e = 0; e < c; ++e)
            if (h.comp[e].id == k.id) return WVN_JPEG_BAD_MARKER;
        }
        if (sampling_of(h) < 0) return WVN_JPEG_UNSUPPORTED;
        h.have_sof = true;
        break;
      }
      case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE:
      case 0xCF: case 0xCC:   // progressive, lossless, hierarchical, arithmetic coding (DAC included)
        return WVN_JPEG_UNSUPPORTED;
      case 0xDC:   // DNL
      case 0xDE:   // DHP
      case 0xDF:   // EXP
        return WVN_JPEG_UNSUPPORTED;
      case 0xDB: {
        int q = 0;
        while (q < sl) {
          const int pq = s[q] >> 4, tq = s[q] & 15;
          if (pq > 1 || tq > 3) return WVN_JPEG_BAD_TABLE;
          const int need = 1 + 64 * (pq + 1);
          if (q + need > sl) return WVN_JPEG_BAD_TABLE;
          for (int i = 0; i < 64; ++i)
            h.qt[tq][kZigzag[i]] = pq ? (uint16_t)be16(s + q + 1 + 2 * i) : s[q + 1 + i];
          h.qt_defined[tq] = true;
          q += need;
        }
        break;
      }
      case 0xC4: {
        int q = 0;
        while (q < sl) {
          if (q + 17 > sl) return WVN_JPEG_BAD_TABLE;
          const int tc = s[q] >> 4, th = s[q] & 15;
          if (tc > 1 || th > 3) return WVN_JPEG_BAD_TABLE;
          int count = 0;
          for (int i = 0; i < 16; ++i) count += s[q + 1 + i];
          if (count > 256 || q + 17 + count > sl) return WVN_JPEG_BAD_TABLE;
          Huff& t = tc ? h.ac[th] : h.dc[th];
          if (build_tables) {
            const int rc = build_huff(t, s + q + 1, s + q + 17, count, tc == 0);
            if (rc) return rc;
          } else {
            t.defined = true;
          }
          q += 17 + count;
        }
        break;
      }
      case 0xDD:
        if (sl != 2) return WVN_JPEG_BAD_MARKER;
        h.restart = be16(s);
        break;
      case 0xE0:
        if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) h.jfif = true;
        break;
      case 0xEE:
        if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
          h.adobe = true;
          h.adobe_transform = s[11];
        }
        break;
      case 0xDA: {
        if (!h.have_sof) return WVN_JPEG_BAD_MARKER;
        if (sl < 1) return WVN_JPEG_BAD_MARKER;
        const int ns = s[0];
        if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return WVN_JPEG_BAD_MARKER;
        if (ns != h.ncomp) return WVN_JPEG_UNSUPPORTED;   // one interleaved scan carries the frame; multi-scan files are refused
        for (int c = 0; c < ns; ++c) {
          if (s[1 + 2 * c] != h.comp[c].id) return WVN_JPEG_UNSUPPORTED;   // (components out of frame order)
          const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
          if (td > 3 || ta > 3) return WVN_JPEG_BAD_TABLE;
          if (!h.dc[td].defined || !h.ac[ta].defined || !h.qt_defined[h.comp[c].tq]) return WVN_JPEG_BAD_TABLE;
          h.comp[c].td = td;
          h.comp[c].ta = ta;
        }
        const uint8_t* e = s + 1 + 2 * ns;
        if (e[0] != 0 || e[1] != 63 || e[2] != 0) return WVN_JPEG_BAD_MARKER;   // Ss, Se, Ah/Al of a sequential scan
        // colour space by libjpeg's rule: JFIF -> YCbCr; else Adobe transform 0 -> RGB; else ids 'R' 'G' 'B' -> RGB
        if (h.ncomp == 3 && !h.jfif) {
          const bool rgb_ids = h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B';
          if (h.adobe ? h.adobe_transform == 0 : rgb_ids) return WVN_JPEG_UNSUPPORTED;
        }
        h.scan = p;
        return WVN_JPEG_OK;
      }
      default:   // APPn, COM and the reserved markers with a length: skipped
        break;
    }
  }
}

void geometry_of(const Header& h, wvn_jpeg_geometry* g) {
  g->width = h.width;
  g->height = h.height;
  g->components = h.ncomp;
  g->sampling = sampling_of(h);
  g->restart_interval = h.restart;
}

// Entropy-coded segment: bytes with FF 00 unstuffed; a marker ends the supply of bits.
struct Bits {
  const uint8_t* d;
  size_t n, p;
  uint64_t acc = 0;   // the low `cnt` bits are valid, most significant first
  int cnt = 0;
  int marker = -1;    // marker met (its FF xx not consumed), or -1
  bool eof = false;

  Bits(const uint8_t* d_, size_t n_, size_t p_) : d(d_), n(n_), p(p_) {}

  void fill() {
    while (cnt <= 56 && marker < 0 && !eof) {
      if (p >= n) { eof = true; break; }
      const uint8_t b = d[p];
      if (b == 0xFF) {
        if (p + 1 >= n) { eof = true; break; }
        const uint8_t b2 = d[p + 1];
        if (b2 == 0) {
          p += 2;
        } else if (b2 == 0xFF) {   // fill byte before a marker
          ++p;
          continue;
        } else {
          marker = b2;
          break;
        }
      } else {
        ++p;
      }
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  // status when `need` bits are not there
  int short_status() const { return (eof || marker == 0xD9) ? WVN_JPEG_TRUNCATED : WVN_JPEG_BAD_MARKER; }
  inline bool ensure(int need) {
    if (cnt < need) fill();
    return cnt >= need;
  }
  inline uint32_t peek(int k) const { return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1u); }
  inline void drop(int k) { cnt -= k; }
};

inline int decode_symbol(Bits& b, const Huff& t, int* sym) {
  b.ensure(16);
  if (b.cnt >= kLook) {
    const uint32_t look = b.peek(kLook);
    const int l = t.look_len[look];
    if (l) {
      b.drop(l);
      *sym = t.look_sym[look];
      return WVN_JPEG_OK;
    }
  }
  // bit by bit (long codes, or fewer than kLook bits left in the segment): a prefix that no shorter length claimed lies at or above
  // the first code of this length, so "<= maxcode" alone identifies a code
  for (int l = 1; l <= 16; ++l) {
    if (b.cnt < l) return b.short_status();
    const int32_t code = (int32_t)b.peek(l);
    if (code <= t.maxcode[l]) {
      const int idx = code + t.valoff[l];
      if (idx < 0 || idx >= t.nsym) return WVN_JPEG_BAD_HUFFMAN;
      b.drop(l);
      *sym = t.huffval[idx];
      return WVN_JPEG_OK;
    }
  }
  return WVN_JPEG_BAD_HUFFMAN;
}

inline int receive_extend(Bits& b, int s, int* v) {
  if (!b.ensure(s)) return b.short_status();
  const int r = (int)b.peek(s);
  b.drop(s);
  *v = (r < (1 << (s - 1))) ? r - (1 << s) + 1 : r;
  return WVN_JPEG_OK;
}

// jidctint.c, one 8-point pass in 64 bits (in and out may not alias)
void islow_pass(const long long* in, long long* out, int shift) {
  long long z2 = in[2], z3 = in[6];
  long long z1 = (z2 + z3) * 4433;
  long long tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
  long long tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const long long half = 1LL << (shift - 1);
  const long long v[8] = {tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3};
  for (int k = 0; k < 8; ++k) {
    const long long t = v[k] + half;
    out[k] = t >= 0 ? t >> shift : -((-t + (1LL << shift) - 1) >> shift);   // floor division, as an arithmetic shift
  }
}

// The range in which libjpeg has ONE answer: its C code (long arithmetic, 10-bit mask behind the IDCT) and its SIMD code (16-bit
// dequantisation, 16-bit saturation between the passes, saturation behind them) agree exactly while every dequantised coefficient
// and every pass-1 value fits int16 and every sample before the + 128 lies in [-512, 511].  Streams encoded from 8-bit pictures
// stay inside (widest sample met: 338, a saturated checkerboard at quality 1); what leaves the range is refused
// (WVN_JPEG_OUT_OF_RANGE), not given one of the two answers.
bool block_in_range(const int16_t* coef, const uint16_t* q) {
  long long deq[64], ws[64], col[8], res[8];
  for (int i = 0; i < 64; ++i) {
    deq[i] = (long long)coef[i] * q[i];
    if (deq[i] < -32768 || deq[i] > 32767) return false;
  }
  for (int u = 0; u < 8; ++u) {
    for (int v = 0; v < 8; ++v) col[v] = deq[8 * v + u];
    islow_pass(col, res, 13 - 2);
    for (int v = 0; v < 8; ++v) {
      if (res[v] < -32768 || res[v] > 32767) return false;
      ws[8 * v + u] = res[v];
    }
  }
  for (int y = 0; y < 8; ++y) {
    islow_pass(ws + 8 * y, res, 13 + 2 + 3);
    for (int x = 0; x < 8; ++x)
      if (res[x] < -512 || res[x] > 511) return false;
  }
  return true;
}

// sum |coef q| up to which block_in_range holds without looking: |pass 1| <= 4 * 1.3871 * sum, |sample| <= 1.3871^2 / 8 * sum (+ rounding)
constexpr long long kSafeL1 = 2000;

int decode_block(Bits& b, const Huff& dc, const Huff& ac, int* pred, int16_t* out, const uint16_t* q, bool* out_of_range) {
  memset(out, 0, 64 * sizeof(int16_t));
  int s, rc, v;
  if ((rc = decode_symbol(b, dc, &s))) return rc;
  if (s > 15) return WVN_JPEG_BAD_HUFFMAN;
  if (s) {
    if ((rc = receive_extend(b, s, &v))) return rc;
    *pred += v;
  }
  if (*pred < -32768 || *pred > 32767) return WVN_JPEG_BAD_COEFFICIENT;
  out[0] = (int16_t)*pred;
  long long l1 = (long long)(*pred < 0 ? -*pred : *pred) * q[0];
  for (int k = 1; k < 64;) {
    int rs;
    if ((rc = decode_symbol(b, ac, &rs))) return rc;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r == 15) { k += 16; if (k > 64) return WVN_JPEG_BAD_COEFFICIENT; continue; }
      if (r != 0) return WVN_JPEG_BAD_HUFFMAN;   // EOBn belongs to progressive scans
      break;
    }
    k += r;
    if (k > 63) return WVN_JPEG_BAD_COEFFICIENT;
    if ((rc = receive_extend(b, s, &v))) return rc;
    out[kZigzag[k]] = (int16_t)v;
    l1 += (long long)(v < 0 ? -v : v) * q[kZigzag[k]];
    ++k;
  }
  if (l1 > kSafeL1 && !block_in_range(out, q)) *out_of_range = true;
  return WVN_JPEG_OK;
}

bool same_geometry(const wvn_jpeg_geometry& a, const wvn_jpeg_geometry& b) {
  return a.width == b.width && a.height == b.height && a.components == b.components && a.sampling == b.sampling;
}

int decode_frame(const uint8_t* d, size_t n, const wvn_jpeg_geometry* expect, const Layout& L, int16_t* coef, uint16_t* qt) {
  // (the tables alone are ~10 KB: on the worker's stack)
  Header h;
  int rc = parse_header(d, n, h, true);
  if (rc) return rc;
  wvn_jpeg_geometry g;
  geometry_of(h, &g);
  if (!same_geometry(g, *expect)) return WVN_JPEG_GEOMETRY_MISMATCH;
  for (int c = 0; c < h.ncomp; ++c) memcpy(qt + 64 * c, h.qt[h.comp[c].tq], 64 * sizeof(uint16_t));
  Bits b(d, n, h.scan);
  int pred[3] = {0, 0, 0};
  bool out_of_range = false;
  int rst = 0;
  long long m = 0;
  for (int my = 0; my < L.mcus_y; ++my) {
    for (int mx = 0; mx < L.mcus_x; ++mx, ++m) {
      if (h.restart && m && m % h.restart == 0) {
        if (b.cnt >= 8) return WVN_JPEG_BAD_MARKER;   // whole bytes left in front of the marker: not skipped, as libjpeg would
        b.cnt = 0;   // the (fewer than 8) padding bits of the interval
        b.acc = 0;
        if (b.marker < 0) b.fill();
        if (b.cnt != 0) return WVN_JPEG_BAD_MARKER;              // data where the RSTn should be
        if (b.marker < 0) return WVN_JPEG_TRUNCATED;
        if (b.marker != 0xD0 + rst) return b.marker == 0xD9 ? WVN_JPEG_TRUNCATED : WVN_JPEG_BAD_MARKER;
        rst = (rst + 1) & 7;
        b.p += 2;
        b.marker = -1;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < L.ncomp; ++c) {
        const Huff& dc = h.dc[h.comp[c].td];
        const Huff& ac = h.ac[h.comp[c].ta];
        const int nh = L.ncomp == 1 ? 1 : L.hs[c], nv = L.ncomp == 1 ? 1 : L.vs[c];
        for (int v = 0; v < nv; ++v)
          for (int u = 0; u < nh; ++u) {
            const long long blk = L.block0[c] + (long long)(my * nv + v) * L.bw[c] + (mx * nh + u);
            if ((rc = decode_block(b, dc, ac, &pred[c], coef + blk * 64, qt + 64 * c, &out_of_range))) return rc;
          }
      }
    }
  }
  // the scan is complete: EOI must follow (fill bytes allowed)
  if (b.cnt >= 8) return WVN_JPEG_BAD_MARKER;
  b.cnt = 0;
  b.acc = 0;
  if (b.marker < 0) b.fill();
  if (b.cnt != 0) return WVN_JPEG_BAD_MARKER;
  if (b.marker < 0) return WVN_JPEG_TRUNCATED;
  if (b.marker != 0xD9) return WVN_JPEG_BAD_MARKER;
  // the range check has the last word: a stream that is also short or corrupt carries that status (tests/jpeg_ref.py: the same order)
  return out_of_range ? WVN_JPEG_OUT_OF_RANGE : WVN_JPEG_OK;
}

}  // namespace

int layout_of(const wvn_jpeg_geometry* g, Layout* L) {
  if (!g || g->width < 1 || g->height < 1 || g->width > WVN_JPEG_MAX_DIM || g->height > WVN_JPEG_MAX_DIM) return WVN_JPEG_BAD_GEOMETRY;
  int H, V;
  switch (g->sampling) {
    case WVN_JPEG_GRAY: H = 1; V = 1; break;
    case WVN_JPEG_444: H = 1; V = 1; break;
    case WVN_JPEG_422: H = 2; V = 1; break;
    case WVN_JPEG_420: H = 2; V = 2; break;
    default: return WVN_JPEG_BAD_GEOMETRY;
  }
  if (g->components != (g->sampling == WVN_JPEG_GRAY ? 1 : 3)) return WVN_JPEG_BAD_GEOMETRY;
  L->ncomp = g->components;
  L->mcus_x = (g->width + 8 * H - 1) / (8 * H);
  L->mcus_y = (g->height + 8 * V - 1) / (8 * V);
  long long blocks = 0, bytes = 0;
  for (int c = 0; c < 3; ++c) {
    const bool live = c < L->ncomp;
    L->hs[c] = c == 0 ? H : 1;
    L->vs[c] = c == 0 ? V : 1;
    L->bw[c] = live ? L->mcus_x * L->hs[c] : 0;
    L->bh[c] = live ? L->mcus_y * L->vs[c] : 0;
    L->cw[c] = live ? (g->width * L->hs[c] + H - 1) / H : 0;
    L->ch[c] = live ? (g->height * L->vs[c] + V - 1) / V : 0;
    L->block0[c] = blocks;
    L->plane0[c] = bytes;
    blocks += (long long)L->bw[c] * L->bh[c];
    bytes += (long long)L->bw[c] * L->bh[c] * 64;
  }
  L->blocks = blocks;
  L->plane_bytes = bytes;
  return WVN_JPEG_OK;
}

int parse_info(const uint8_t* data, size_t n, wvn_jpeg_geometry* g) {
  // the whole header is walked (tables, SOS): a frame that `info` accepts is refused later only for its entropy-coded data
  Header h;   // (~12 KB: on the stack, nothing here allocates)
  const int rc = parse_header(data, n, h, true);
  if (rc == WVN_JPEG_OK) geometry_of(h, g);
  return rc;
}

void probe_batch(const void* const* data, const size_t* sizes, int B, wvn_jpeg_geometry* g, int* status) {
  for (int b = 0; b < B; ++b) {
    Header h;
    g[b] = wvn_jpeg_geometry{0, 0, 0, 0, 0};
    status[b] = parse_header((const uint8_t*)data[b], sizes[b], h, false);
    if (status[b] == WVN_JPEG_OK) geometry_of(h, &g[b]);
  }
}

int decode_coefficients(const uint8_t* data, size_t n, const wvn_jpeg_geometry* expect, int16_t* coef, uint16_t* qt) {
  Layout L;
  int rc = layout_of(expect, &L);
  if (rc) return rc;
  memset(qt, 0, 3 * 64 * sizeof(uint16_t));
  rc = decode_frame(data, n, expect, L, coef, qt);
  if (rc) {
    memset(coef, 0, (size_t)L.blocks * 64 * sizeof(int16_t));
    memset(qt, 0, 3 * 64 * sizeof(uint16_t));
  }
  return rc;
}

void decode_batch_host(const void* const* data, const size_t* sizes, int B, const wvn_jpeg_geometry* g, int16_t* coef, size_t coef_stride,
                       uint16_t* qt, size_t qt_stride, int threads, int* status) {
  if (threads < 1) threads = 1;
  if (threads > WVN_JPEG_MAX_THREADS) threads = WVN_JPEG_MAX_THREADS;
  if (threads > B) threads = B;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1))
      status[b] = decode_coefficients((const uint8_t*)data[b], sizes[b], g, coef + (size_t)b * coef_stride, qt + (size_t)b * qt_stride);
  };
  // a worker that cannot be started (no memory, no thread) is not an error: the others and the caller take its frames
  std::vector<std::thread> pool;
  try {
    pool.reserve((size_t)threads);
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  } catch (...) {
  }
  work();   // the caller is worker 0
  for (auto& t : pool) t.join();
}

}  // namespace wvn_jpeg
