"""The JPEG ingest stated in numpy: the definition ops.jpeg_decode is held to (include/wvn_hip.h: "JPEG ingest").

Baseline / extended sequential Huffman JPEG with 8-bit samples, one interleaved scan; grayscale, 4:4:4, 4:2:2 and 4:2:0.
The pixel stages are libjpeg's with its default settings, operation by operation in integers (32 bits suffice):
    jidctint.c  jpeg_idct_islow       dequantise, two 8-point passes with 13-bit constants, + 128, range limit
    jdsample.c  h2v1 / h2v2 fancy     triangle filter, with the edge rules on the component's real size
    jdcolor.c   ycc_rgb_convert       16-bit fixed-point tables
tests/test_jpeg_host.py pins `decode` to Pillow (libjpeg-turbo) at zero differing bytes.  Written for clarity, not speed.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

STATUS = ("OK", "TRUNCATED", "BAD_MARKER", "BAD_TABLE", "BAD_HUFFMAN", "BAD_COEFFICIENT", "UNSUPPORTED", "GEOMETRY_MISMATCH",
          "BAD_GEOMETRY", "OUT_OF_RANGE")
SAMPLING = {(1, 1, 1): "gray", (3, 1, 1): "4:4:4", (3, 2, 1): "4:2:2", (3, 2, 2): "4:2:0"}


class JpegError(ValueError):
    """args[0] is the name of the status the library gives the same stream."""


# ---------------------------------------------------------------------------------------------------------------- header
class Frame:
    pass


def _huffman_table(bits, vals, is_dc):
    """{(length, code): symbol} of the canonical code (T.81 annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if code + n > (1 << length):
            raise JpegError("BAD_TABLE")
        for _ in range(n):
            if is_dc and vals[k] > 15:
                raise JpegError("BAD_TABLE")
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def parse(data) -> Frame:
    d = bytes(data)
    n = len(d)
    if n < 2:
        raise JpegError("TRUNCATED")
    if d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError("BAD_MARKER")
    f = Frame()
    f.qt, f.dc, f.ac, f.restart, f.comps = {}, {}, {}, 0, None
    jfif = adobe = False
    adobe_transform = 0
    p = 2
    while True:
        if p >= n:
            raise JpegError("TRUNCATED")
        if d[p] != 0xFF:
            raise JpegError("BAD_MARKER")
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            raise JpegError("TRUNCATED")
        m = d[p]
        p += 1
        if m == 0xD9:
            raise JpegError("TRUNCATED")
        if m in (0, 1) or 0xD0 <= m <= 0xD8:
            raise JpegError("BAD_MARKER")
        if p + 2 > n:
            raise JpegError("TRUNCATED")
        length = (d[p] << 8) | d[p + 1]
        if length < 2:
            raise JpegError("BAD_MARKER")
        if p + length > n:
            raise JpegError("TRUNCATED")
        s = d[p + 2:p + length]
        p += length
        if m in (0xC0, 0xC1):
            if f.comps is not None or len(s) < 6:
                raise JpegError("BAD_MARKER")
            if s[0] != 8:
                raise JpegError("UNSUPPORTED")
            f.height, f.width, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if len(s) != 6 + 3 * nc:
                raise JpegError("BAD_MARKER")
            if nc not in (1, 3) or f.height == 0 or f.width == 0 or max(f.height, f.width) > 16384:
                raise JpegError("UNSUPPORTED")
            comps = [dict(id=s[6 + 3 * c], h=s[7 + 3 * c] >> 4, v=s[7 + 3 * c] & 15, tq=s[8 + 3 * c]) for c in range(nc)]
            for c, k in enumerate(comps):
                if not (1 <= k["h"] <= 4 and 1 <= k["v"] <= 4) or k["id"] in [e["id"] for e in comps[:c]]:
                    raise JpegError("BAD_MARKER")
                if k["tq"] > 3:
                    raise JpegError("BAD_TABLE")
            if nc == 3 and ([(k["h"], k["v"]) for k in comps[1:]] != [(1, 1)] * 2 or (3, comps[0]["h"], comps[0]["v"]) not in SAMPLING):
                raise JpegError("UNSUPPORTED")
            f.comps = comps
        elif 0xC2 <= m <= 0xCF and m != 0xC4 or m in (0xDC, 0xDE, 0xDF):
            raise JpegError("UNSUPPORTED")
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                need = 1 + 64 * (pq + 1)
                if pq > 1 or tq > 3 or q + need > len(s):
                    raise JpegError("BAD_TABLE")
                raw = s[q + 1:q + need]
                zz = [(raw[2 * i] << 8) | raw[2 * i + 1] for i in range(64)] if pq else list(raw)
                table = np.zeros(64, np.int32)
                table[ZIGZAG] = zz          # the file carries zigzag order; everything below is in natural order
                f.qt[tq] = table
                q += need
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    raise JpegError("BAD_TABLE")
                tc, th = s[q] >> 4, s[q] & 15
                bits = list(s[q + 1:q + 17])
                if tc > 1 or th > 3 or sum(bits) > 256 or q + 17 + sum(bits) > len(s):
                    raise JpegError("BAD_TABLE")
                (f.ac if tc else f.dc)[th] = _huffman_table(bits, s[q + 17:q + 17 + sum(bits)], tc == 0)
                q += 17 + sum(bits)
        elif m == 0xDD:
            if len(s) != 2:
                raise JpegError("BAD_MARKER")
            f.restart = (s[0] << 8) | s[1]
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe, adobe_transform = True, s[11]
        elif m == 0xDA:
            if f.comps is None or len(s) < 1:
                raise JpegError("BAD_MARKER")
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) != 4 + 2 * ns:
                raise JpegError("BAD_MARKER")
            if ns != len(f.comps):
                raise JpegError("UNSUPPORTED")
            for c, k in enumerate(f.comps):
                if s[1 + 2 * c] != k["id"]:
                    raise JpegError("UNSUPPORTED")
                k["td"], k["ta"] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if k["td"] > 3 or k["ta"] > 3 or k["td"] not in f.dc or k["ta"] not in f.ac or k["tq"] not in f.qt:
                    raise JpegError("BAD_TABLE")
            if tuple(s[1 + 2 * ns:]) != (0, 63, 0):
                raise JpegError("BAD_MARKER")
            if len(f.comps) == 3 and not jfif:   # libjpeg's colour-space rule: these files hold RGB, not YCbCr
                ids = bytes(k["id"] for k in f.comps)
                if (adobe_transform == 0) if adobe else ids == b"RGB":
                    raise JpegError("UNSUPPORTED")
            f.scan = p
            break
    nc = len(f.comps)
    if nc == 1:
        f.comps[0]["h"] = f.comps[0]["v"] = 1    # one component: the scan is not interleaved, its factors mean nothing
    f.hmax, f.vmax = f.comps[0]["h"], f.comps[0]["v"]
    f.sampling = SAMPLING[(nc, f.hmax, f.vmax)]
    f.mcus_x = -(-f.width // (8 * f.hmax))
    f.mcus_y = -(-f.height // (8 * f.vmax))
    for k in f.comps:
        k["bw"], k["bh"] = f.mcus_x * k["h"], f.mcus_y * k["v"]
        k["cw"] = -(-f.width * k["h"] // f.hmax)     # the component's real size in samples
        k["ch"] = -(-f.height * k["v"] // f.vmax)
    return f


# ---------------------------------------------------------------------------------------------------------------- entropy decoder
class _Bits:
    """The entropy-coded segment bit by bit: FF 00 is the byte FF, FF FF is fill, any other FF xx is a marker and ends the bits."""

    def __init__(self, d, p):
        self.d, self.p, self.acc, self.cnt, self.marker = d, p, 0, 0, None

    def _byte(self):
        d = self.d
        while True:
            if self.marker is not None:
                raise JpegError("TRUNCATED" if self.marker == 0xD9 else "BAD_MARKER")
            if self.p >= len(d):
                raise JpegError("TRUNCATED")
            b = d[self.p]
            if b != 0xFF:
                self.p += 1
                return b
            if self.p + 1 >= len(d):
                raise JpegError("TRUNCATED")
            b2 = d[self.p + 1]
            if b2 == 0:
                self.p += 2
                return 0xFF
            if b2 == 0xFF:
                self.p += 1
                continue
            self.marker = b2

    def bit(self):
        if self.cnt == 0:
            self.acc, self.cnt = self._byte(), 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def next_marker(self):
        """Drop the padding bits; the marker that follows (None: more data follows instead)."""
        self.cnt = 0
        if self.marker is None:
            try:
                self._byte()
            except JpegError:
                if self.marker is None:
                    raise
            else:
                raise JpegError("BAD_MARKER")
        return self.marker


def _symbol(b, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | b.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise JpegError("BAD_HUFFMAN")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _block(b, dc, ac, pred):
    out = np.zeros(64, np.int16)
    s = _symbol(b, dc)
    if s:
        pred += _extend(b.bits(s), s)
    if not -32768 <= pred <= 32767:
        raise JpegError("BAD_COEFFICIENT")
    out[0] = pred
    k = 1
    while k < 64:
        rs = _symbol(b, ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                k += 16
                if k > 64:
                    raise JpegError("BAD_COEFFICIENT")
                continue
            if r:
                raise JpegError("BAD_HUFFMAN")
            break
        k += r
        if k > 63:
            raise JpegError("BAD_COEFFICIENT")
        out[ZIGZAG[k]] = _extend(b.bits(s), s)
        k += 1
    return out, pred


def coefficients(data):
    """(frame, [int16 [bh, bw, 64] per component]): quantised coefficients in natural order, each component padded to whole MCUs."""
    d = bytes(data)
    f = parse(d)
    coef = [np.zeros((k["bh"], k["bw"], 64), np.int16) for k in f.comps]
    b = _Bits(d, f.scan)
    pred = [0] * len(f.comps)
    rst = 0
    for m in range(f.mcus_x * f.mcus_y):
        my, mx = divmod(m, f.mcus_x)
        if f.restart and m and m % f.restart == 0:
            marker = b.next_marker()
            if marker != 0xD0 + rst:
                raise JpegError("TRUNCATED" if marker == 0xD9 else "BAD_MARKER")
            rst = (rst + 1) & 7
            b.p += 2
            b.marker = None
            pred = [0] * len(f.comps)
        for c, k in enumerate(f.comps):
            for v in range(k["v"]):
                for u in range(k["h"]):
                    coef[c][my * k["v"] + v, mx * k["h"] + u], pred[c] = _block(b, f.dc[k["td"]], f.ac[k["ta"]], pred[c])
    if b.next_marker() != 0xD9:
        raise JpegError("BAD_MARKER")
    return f, coef


def coefficients_flat(data):
    """The library's layout: int16 [blocks, 64], component after component, and uint16 [3, 64] quantisation tables."""
    f, coef = coefficients(data)
    qt = np.zeros((3, 64), np.uint16)
    for c, k in enumerate(f.comps):
        qt[c] = f.qt[k["tq"]]
    return f, np.concatenate([c.reshape(-1, 64) for c in coef]), qt


# ---------------------------------------------------------------------------------------------------------------- inverse DCT
def _islow_pass(x, shift):
    """jpeg_idct_islow, one 8-point pass along the last axis, descaled by `shift` with round-half-up.  Exact (int64): inside the
    range idct_blocks accepts every intermediate fits 32 bits, so this is also what 32-bit registers give."""
    x = x.astype(np.int64)
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2 = z1 + i6 * -15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (shift - 1)
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(o + half) >> shift for o in out], axis=-1)


def _outside(a, lo, hi):
    return a.size > 0 and (a.min() < lo or a.max() > hi)


def idct_blocks(coef, qt):
    """coef int16 [..., 64], qt [64] (natural order) -> samples uint8 [..., 8, 8].

    OUT_OF_RANGE: libjpeg's C code (long arithmetic, a 10-bit mask behind the IDCT) and its SIMD code (16-bit dequantisation, 16-bit
    saturation between the passes and behind them) agree while every dequantised coefficient and every pass-1 value fits int16 and
    every sample before the + 128 lies in [-512, 511] -- inside that range 32-bit arithmetic is exact, too.  Outside it libjpeg has
    two answers and the frame is refused.  Streams encoded from 8-bit pictures stay inside (the widest sample met: 338, a saturated checkerboard at quality 1)."""
    deq = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))         # [v, u]
    cols = _islow_pass(np.swapaxes(deq, -1, -2), 13 - 2)                # pass 1 runs down the columns: [u, y]
    rows = _islow_pass(np.swapaxes(cols, -1, -2), 13 + 2 + 3)           # pass 2 along the rows: [y, x]
    if _outside(deq, -32768, 32767) or _outside(cols, -32768, 32767) or _outside(rows, -512, 511):
        raise JpegError("OUT_OF_RANGE")
    v = rows & 1023                                                     # range_limit[x & RANGE_MASK] of libjpeg
    v = np.where(v >= 512, v - 1024, v) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def planes(data):
    """(frame, [uint8 [bh 8, bw 8] per component]): the component planes at component resolution, padding included."""
    f, coef = coefficients(data)
    out = []
    for k, c in zip(f.comps, coef):
        s = idct_blocks(c, f.qt[k["tq"]])                               # [bh, bw, 8, 8]
        out.append(s.transpose(0, 2, 1, 3).reshape(k["bh"] * 8, k["bw"] * 8))
    return f, out


# ---------------------------------------------------------------------------------------------------------------- upsampling
def _fancy_h(t, near_w, round_even, round_odd, shift):
    """Triangle filter along x on sums t (int32 [rows, cw]): out[2i] = (near_w t[i] + t[i-1] + round_even) >> shift, out[2i+1] likewise
    with t[i+1]; at either end the missing neighbour is the sample itself."""
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int32)
    out[:, 0::2] = (near_w * t + left + round_even) >> shift
    out[:, 1::2] = (near_w * t + right + round_odd) >> shift
    return out


def upsample(plane, cw, ch, hfac, vfac):
    """plane: the component's REAL samples are plane[:ch, :cw] -> int32 [ch vfac, cw hfac] (libjpeg's fancy upsampling; a component
    of real width <= 2 is replicated, as libjpeg does there)."""
    s = plane[:ch, :cw].astype(np.int32)
    if hfac == 1 and vfac == 1:
        return s
    if cw <= 2:
        return np.repeat(np.repeat(s, vfac, axis=0), hfac, axis=1)
    if vfac == 1:                                                        # h2v1: 3/4, 1/4 with + 1 / + 2
        return _fancy_h(s, 3, 1, 2, 2)
    above = np.concatenate([s[:1], s[:-1]], axis=0)                      # the first and the last real row stand in for
    below = np.concatenate([s[1:], s[-1:]], axis=0)                      # the rows beyond them
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[0::2] = _fancy_h(3 * s + above, 3, 8, 7, 4)                      # h2v2: 9/16, 3/16, 3/16, 1/16 with + 8 / + 7
    out[1::2] = _fancy_h(3 * s + below, 3, 8, 7, 4)
    return out


# ---------------------------------------------------------------------------------------------------------------- colour
def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)


def decode(data, gray=False):
    """bytes -> uint8 [3, H, W] RGB ([1, H, W] with gray=True, one-component files only)."""
    f, pl = planes(data)
    H, W = f.height, f.width
    if len(pl) == 1:
        y = pl[0][:H, :W]
        return y[None].copy() if gray else np.stack([y, y, y])
    if gray:
        raise JpegError("BAD_GEOMETRY")
    cb, cr = (upsample(p, k["cw"], k["ch"], f.hmax, f.vmax)[:H, :W] for p, k in zip(pl[1:], f.comps[1:]))
    return ycc_to_rgb(pl[0][:H, :W], cb, cr)
