"""The rule book of lossy WebP (one VP8 key frame, RFC 6386, and libwebp's YUV -> RGB tail) in NumPy and plain Python: what
maf-yolo_amd/webp_lossy.py and csrc/vp8_decode.hip must compute, bit for bit.  tools/make_golden_webp_lossy.py asserts that it equals Pillow
(libwebp) and WebPDecodeYUV on every fixture; the tests compare the device with the fixtures and this file with both.

  decode_stages(d) -> (bgr uint8 [h, w, 3], (Y, U, V) uint8 planes cropped to w x h and ceil(w / 2) x ceil(h / 2), status)
  describe(d)      -> Frame: the header fields, the per-macroblock modes and the coefficient LEVELS (before dequantisation)
  transcode(d, **changes) -> a new file with the same modes and levels and a changed header (Pillow's encoder sets none of these fields)
  BoolEncoder, write_frame: the writer behind transcode.

The syntax is written ONCE (walk_header, walk_modes, walk_coeffs) over an `io` that either reads bools (BoolDecoder) or writes them
(BoolEncoder): a reader ignores the value it is handed and returns what the stream says, a writer writes the value and returns it.

The bool decoder loads LAZILY, as libwebp's does: a byte is fetched only when a bool starts with fewer than 8 unread bits, and
STATUS_INPUT_EXHAUSTED means that such a fetch found its partition at its end (libwebp's eof_, which fails the decode).  The flush bytes an
encoder appends are therefore never needed.  STATUS_BAD_PARTITIONS: the partition size table does not fit behind the first partition, or the
sizes leave the LAST partition empty (libwebp clamps every size to what is left and then refuses exactly that).

Coefficients are stored as int16, as libwebp stores them.  Beyond +-2047 libwebp's C and SIMD transforms are not promised to agree, so there
is no judge for a hand-made case out there: the fixture tool keeps every dequantised coefficient of a transcoded case inside that range, and
nothing here is claimed beyond it.
"""
import struct
from collections import Counter

import numpy as np

from webp_lossy_tables import AC_Q, BANDS, BMODE_PROBA, CAT3456, COEFF_PROBA0, COEFF_UPDATE, DC_Q, ZIGZAG

STATUS_INPUT_EXHAUSTED, STATUS_BAD_PARTITIONS = 1, 2
DC_PRED, TM_PRED, V_PRED, H_PRED = 0, 1, 2, 3
B_DC, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU = range(10)

counters = Counter()          # coverage: which paths the decodes since the last counters.clear() reached (the fixture tool asserts on it)


# ---------------------------------------------------------------- bools

class BoolDecoder:
    encoding = False

    def __init__(self, buf, start, end):
        self.buf, self.pos, self.end = buf, start, end
        self.value, self.range, self.bits, self.eof = 0, 254, -8, False          # range is kept minus one

    def _load(self):
        if self.pos < self.end:
            self.value = (self.value << 8) | self.buf[self.pos]
            self.pos += 1
            self.bits += 8
        elif not self.eof:
            self.value <<= 8
            self.bits += 8
            self.eof = True
        else:
            self.bits = 0

    def bit(self, prob, _=None):
        r = self.range
        if self.bits < 0:
            self._load()
        pos = self.bits
        split = (r * prob) >> 8
        if (self.value >> pos) > split:
            r -= split
            self.value -= (split + 1) << pos
            b = 1
        else:
            r = split + 1
            b = 0
        shift = 7 ^ (r.bit_length() - 1)
        self.bits -= shift
        self.range = (r << shift) - 1
        return b


class BoolEncoder:
    """RFC 6386 section 7.3."""
    encoding = True

    def __init__(self):
        self.out, self.range, self.bottom, self.count = bytearray(), 255, 0, 24

    def _carry(self):
        i = len(self.out) - 1
        while self.out[i] == 255:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def bit(self, prob, b):
        b = 1 if b else 0
        split = 1 + (((self.range - 1) * prob) >> 8)
        if b:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                self._carry()
            self.bottom = (self.bottom << 1) & 0xffffffff
            self.count -= 1
            if not self.count:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.count = 8
        return b

    def finish(self):
        c, v = self.count, self.bottom
        if v & (1 << (32 - c)):
            self._carry()
        v = (v << (c & 7)) & 0xffffffff
        for _ in range(c >> 3):
            v = (v << 8) & 0xffffffff
        for _ in range(4):
            self.out.append(v >> 24)
            v = (v << 8) & 0xffffffff
        return bytes(self.out)


def _value(io, n, x=None):
    v = 0
    for i in range(n - 1, -1, -1):
        v = 2 * v + io.bit(128, None if x is None else (x >> i) & 1)
    return v


def _signed(io, n, x=None):
    v = _value(io, n, None if x is None else abs(x))
    return -v if io.bit(128, None if x is None else x < 0) else v


def _opt_signed(io, n, x):
    """flag ? signed value : 0"""
    e = io.encoding
    return _signed(io, n, x if e else None) if io.bit(128, x != 0 if e else None) else 0


# ---------------------------------------------------------------- the frame header (first partition)

class Frame:
    """Header fields (defaults: what a key frame starts from), then mbs: one dict per macroblock in raster order."""

    def __init__(self):
        self.width = self.height = 0
        self.xscale = self.yscale = 0
        self.colorspace = self.clamp = 0
        self.use_segment = self.update_map = self.update_data = self.absolute = 0
        self.seg_quant, self.seg_filter, self.seg_proba = [0] * 4, [0] * 4, [255] * 3
        self.simple = self.level = self.sharpness = 0
        self.use_lf_delta = self.lf_update = 0
        self.ref_delta, self.mode_delta = [0] * 4, [0] * 4
        self.log2_parts = 0
        self.base_q = 0
        self.dq = [0] * 5                      # y1_dc, y2_dc, y2_ac, uv_dc, uv_ac
        self.refresh = 0
        self.proba = COEFF_PROBA0.copy()
        self.use_skip, self.skip_proba = 0, 0
        self.mbs = []

    @property
    def mbw(self):
        return (self.width + 15) >> 4

    @property
    def mbh(self):
        return (self.height + 15) >> 4


def walk_header(io, f):
    """Everything of the first partition in front of the macroblock modes, but for the partition count (walk_partitions reads it between
    the filter header and the quantisers)."""
    e = io.encoding

    def g(x):
        return x if e else None
    f.colorspace = io.bit(128, g(f.colorspace))
    f.clamp = io.bit(128, g(f.clamp))
    f.use_segment = io.bit(128, g(f.use_segment))
    if f.use_segment:
        f.update_map = io.bit(128, g(f.update_map))
        f.update_data = io.bit(128, g(f.update_data))
        if f.update_data:
            f.absolute = io.bit(128, g(f.absolute))
            f.seg_quant = [_opt_signed(io, 7, x) for x in f.seg_quant]
            f.seg_filter = [_opt_signed(io, 6, x) for x in f.seg_filter]
        if f.update_map:
            f.seg_proba = [_value(io, 8, g(x)) if io.bit(128, x != 255 if e else None) else 255 for x in f.seg_proba]
    else:
        f.update_map = 0
    f.simple = io.bit(128, g(f.simple))
    f.level = _value(io, 6, g(f.level))
    f.sharpness = _value(io, 3, g(f.sharpness))
    f.use_lf_delta = io.bit(128, g(f.use_lf_delta))
    if f.use_lf_delta:
        f.lf_update = io.bit(128, g(f.lf_update))
        if f.lf_update:
            for arr in (f.ref_delta, f.mode_delta):
                for i in range(4):
                    if io.bit(128, arr[i] != 0 if e else None):
                        arr[i] = _signed(io, 6, g(arr[i]))
    f.log2_parts = _value(io, 2, g(f.log2_parts))


def walk_header_tail(io, f):
    e = io.encoding

    def g(x):
        return x if e else None
    f.base_q = _value(io, 7, g(f.base_q))
    f.dq = [_opt_signed(io, 4, x) for x in f.dq]
    f.refresh = io.bit(128, g(f.refresh))                                        # read and ignored
    new = f.proba.copy()
    for t in range(4):
        for b in range(8):
            for c in range(3):
                for p in range(11):
                    want = int(f.proba[t, b, c, p])
                    if io.bit(int(COEFF_UPDATE[t, b, c, p]), want != int(COEFF_PROBA0[t, b, c, p]) if e else None):
                        new[t, b, c, p] = _value(io, 8, g(want))
                    else:
                        new[t, b, c, p] = COEFF_PROBA0[t, b, c, p]
    f.proba = new
    f.use_skip = io.bit(128, g(f.use_skip))
    if f.use_skip:
        f.skip_proba = _value(io, 8, g(f.skip_proba))


def quantisers(f):
    """Per segment (y1_dc, y1_ac, y2_dc, y2_ac, uv_dc, uv_ac), and the quantiser indices used (for the coverage counters)."""
    out = []
    for s in range(4):
        if f.use_segment:
            q = f.seg_quant[s] + (0 if f.absolute else f.base_q)
        else:
            q = f.base_q

        def ix(d, hi=127):
            return min(max(q + d, 0), hi)
        y2ac = (int(AC_Q[ix(f.dq[2])]) * 101581) >> 16
        out.append((int(DC_Q[ix(f.dq[0])]), int(AC_Q[ix(0)]), int(DC_Q[ix(f.dq[1])]) * 2, max(y2ac, 8), int(DC_Q[ix(f.dq[3], 117)]), int(AC_Q[ix(f.dq[4])]),
                    (ix(f.dq[0]), ix(0), ix(f.dq[1]), ix(f.dq[2]), ix(f.dq[3], 117), ix(f.dq[4]))))
    return out


def filter_strengths(f):
    """[segment][is 4x4] -> (limit, interior level, hev threshold); limit 0: no filtering."""
    out = []
    for s in range(4):
        base = f.seg_filter[s] + (0 if f.absolute else f.level) if f.use_segment else f.level
        row = []
        for i4 in (0, 1):
            lv = base
            if f.use_lf_delta:
                lv += f.ref_delta[0]
                if i4:
                    lv += f.mode_delta[0]
            lv = min(max(lv, 0), 63)
            if lv > 0:
                il = lv
                if f.sharpness > 0:
                    il >>= 2 if f.sharpness > 4 else 1
                    il = min(il, 9 - f.sharpness)
                il = max(il, 1)
                row.append((2 * lv + il, il, 2 if lv >= 40 else 1 if lv >= 15 else 0))
            else:
                row.append((0, 0, 0))
        out.append(row)
    return out


# ---------------------------------------------------------------- macroblock modes and tokens

def walk_modes(io, f, mb, top, left):
    """One macroblock's modes from the first partition.  top: the 4 sub-modes above (of this macroblock column), left: the 4 to the left."""
    e = io.encoding
    if f.update_map:
        s = mb.get("segment", 0)
        if not io.bit(f.seg_proba[0], s >= 2 if e else None):
            mb["segment"] = io.bit(f.seg_proba[1], s & 1 if e else None)
        else:
            mb["segment"] = 2 + io.bit(f.seg_proba[2], s & 1 if e else None)
    else:
        mb["segment"] = 0
    mb["skip"] = io.bit(f.skip_proba, mb.get("skip", 0) if e else None) if f.use_skip else 0
    mb["i4"] = 0 if io.bit(145, not mb["i4"] if e else None) else 1
    if not mb["i4"]:
        m = mb["ymode"] if e else 0
        if io.bit(156, m in (TM_PRED, H_PRED) if e else None):
            m = TM_PRED if io.bit(128, m == TM_PRED if e else None) else H_PRED
        else:
            m = V_PRED if io.bit(163, m == V_PRED if e else None) else DC_PRED
        mb["ymode"] = m
        top[:] = [m] * 4
        left[:] = [m] * 4
    else:
        modes = list(mb["modes"]) if e else [0] * 16
        for y in range(4):
            for x in range(4):
                p = [int(v) for v in BMODE_PROBA[top[x], left[y]]]
                m = modes[4 * y + x]

                def b(i, val):
                    return io.bit(p[i], val if e else None)
                if not b(0, m != B_DC):
                    m = B_DC
                elif not b(1, m != B_TM):
                    m = B_TM
                elif not b(2, m != B_VE):
                    m = B_VE
                elif not b(3, m in (B_LD, B_VL, B_HD, B_HU)):
                    m = B_HE if not b(4, m != B_HE) else (B_RD if not b(5, m != B_RD) else B_VR)
                else:
                    m = B_LD if not b(6, m != B_LD) else (B_VL if not b(7, m != B_VL) else (B_HD if not b(8, m != B_HD) else B_HU))
                modes[4 * y + x] = top[x] = left[y] = m
        mb["modes"] = modes
    u = mb["uvmode"] if e else 0
    if not io.bit(142, u != DC_PRED if e else None):
        u = DC_PRED
    elif not io.bit(114, u != V_PRED if e else None):
        u = V_PRED
    else:
        u = TM_PRED if io.bit(183, u == TM_PRED if e else None) else H_PRED
    mb["uvmode"] = u


def _large(io, p, a):
    e = io.encoding

    def b(prob, val):
        return io.bit(prob, val if e else None)
    if not b(p[3], a > 4):
        if not b(p[4], a > 2):
            return 2
        return 3 + b(p[5], a == 4)
    if not b(p[6], a > 10):
        if not b(p[7], a > 6):
            return 5 + b(159, a == 6)
        v = 7 + 2 * b(165, a >= 9)
        return v + b(145, (a - 7) & 1)
    cat = (0 if a < 19 else 1 if a < 35 else 2 if a < 67 else 3) if e else 0
    bit1 = b(p[8], cat >= 2)
    cat = 2 * bit1 + b(p[9 + bit1], cat & 1)
    tab = CAT3456[cat]
    extra = a - 3 - (8 << cat) if e else 0
    v = 0
    for i, pr in enumerate(tab):
        v = 2 * v + b(pr, (extra >> (len(tab) - 1 - i)) & 1)
    return v + 3 + (8 << cat)


def _token_name(v):
    v = abs(v)
    return ("tok%d" % v if v <= 4 else "cat1" if v <= 6 else "cat2" if v <= 10 else "cat3" if v <= 18 else "cat4" if v <= 34 else "cat5" if v <= 66
            else "cat6")


def walk_coeffs(io, P, ctx, n, lv):
    """The tokens of one block.  P: proba[type]; lv: 16 levels in zigzag order (read: filled; written: taken) -> one past the last non-zero."""
    e = io.encoding
    last = max([i + 1 for i in range(n, 16) if lv[i]], default=n) if e else 0
    p = P[BANDS[n]][ctx]
    while n < 16:
        if not io.bit(int(p[0]), n < last if e else None):
            counters["tok_eob"] += 1
            return n
        while not io.bit(int(p[1]), lv[n] != 0 if e else None):
            counters["tok0"] += 1
            n += 1
            p = P[BANDS[n]][0]
            if n == 16:
                return 16
        a = abs(lv[n]) if e else 0
        if not io.bit(int(p[2]), a > 1 if e else None):
            v, nxt = 1, 1
        else:
            v, nxt = _large(io, [int(q) for q in p], a), 2
        lv[n] = -v if io.bit(128, lv[n] < 0 if e else None) else v
        counters[_token_name(v)] += 1
        n += 1
        p = P[BANDS[n]][nxt]
    return 16


def walk_residuals(io, f, mb, top_nz, left_nz):
    """The tokens of one macroblock from its row's token partition.  levels: [25][16] in zigzag order, block 24 = Y2.
    top_nz / left_nz: [9] flags (4 Y, 2 U, 2 V, Y2) of this macroblock column / row."""
    e = io.encoding
    lv = mb["levels"] if e else [[0] * 16 for _ in range(25)]
    nzs = [0] * 25
    if not mb["i4"]:
        nz = walk_coeffs(io, f.proba[1], top_nz[8] + left_nz[8], 0, lv[24])
        top_nz[8] = left_nz[8] = int(nz > 0)
        nzs[24] = nz
        first, t = 1, 0
    else:
        first, t = 0, 3
    for y in range(4):
        for x in range(4):
            nz = walk_coeffs(io, f.proba[t], top_nz[x] + left_nz[y], first, lv[4 * y + x])
            top_nz[x] = left_nz[y] = int(nz > first)
            nzs[4 * y + x] = nz
    for ch in (0, 1):
        for y in range(2):
            for x in range(2):
                i = 4 + 2 * ch
                nz = walk_coeffs(io, f.proba[2], top_nz[i + x] + left_nz[i + y], 0, lv[16 + 4 * ch + 2 * y + x])
                top_nz[i + x] = left_nz[i + y] = int(nz > 0)
                nzs[16 + 4 * ch + 2 * y + x] = nz
    mb["levels"], mb["nz"] = lv, nzs


def walk_frame(io0, ios, f, reading):
    """All macroblocks: modes from io0, tokens from ios[row & (n - 1)]."""
    mbw, mbh = f.mbw, f.mbh
    top_modes = [[B_DC] * 4 for _ in range(mbw)]
    top_nz = [[0] * 9 for _ in range(mbw)]
    if reading:
        f.mbs = [dict() for _ in range(mbw * mbh)]
    for my in range(mbh):
        left_modes, left_nz = [B_DC] * 4, [0] * 9
        io = ios[my & (len(ios) - 1)]
        for mx in range(mbw):
            mb = f.mbs[my * mbw + mx]
            walk_modes(io0, f, mb, top_modes[mx], left_modes)
            if not mb["skip"]:
                walk_residuals(io, f, mb, top_nz[mx], left_nz)
            else:
                keep_t, keep_l = top_nz[mx][8], left_nz[8]
                top_nz[mx][:] = [0] * 9
                left_nz[:] = [0] * 9
                if mb["i4"]:
                    top_nz[mx][8], left_nz[8] = keep_t, keep_l
                if reading or "levels" not in mb:
                    mb["levels"], mb["nz"] = [[0] * 16 for _ in range(25)], [0] * 25


# ---------------------------------------------------------------- container

def vp8_payload(d):
    """(begin, end) of the payload of the first `VP8 ` chunk of a RIFF / WEBP file."""
    assert d[:4] == b"RIFF" and d[8:12] == b"WEBP"
    end = min(len(d), 8 + struct.unpack("<I", d[4:8])[0])
    p = 12
    while p + 8 <= end:
        L, = struct.unpack("<I", d[p + 4:p + 8])
        if d[p:p + 4] == b"VP8 ":
            return p + 8, min(p + 8 + L, end)
        p += 8 + L + (L & 1)
    raise ValueError("no VP8 chunk")


def riff(payload, extra=b""):
    """A bare RIFF / WEBP file around one `VP8 ` payload."""
    body = b"WEBP" + extra + b"VP8 " + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def replace_payload(d, payload):
    """The file `d` with the payload of its `VP8 ` chunk replaced (chunk and RIFF sizes patched; every other chunk kept)."""
    s, e = vp8_payload(d)
    e_padded = e + ((e - s) & 1)
    body = d[8:s - 4] + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"") + d[e_padded:]
    return b"RIFF" + struct.pack("<I", len(body)) + body


# ---------------------------------------------------------------- reading a frame

def describe(d):
    """-> (Frame, status, partition table [(begin, end)] in file offsets: the first partition, then the token partitions)."""
    d = bytes(d)
    s, e = vp8_payload(d)
    tag = d[s] | d[s + 1] << 8 | d[s + 2] << 16
    assert not tag & 1 and tag >> 4 & 1 and d[s + 3:s + 6] == b"\x9d\x01\x2a", "not a visible key frame"
    f = Frame()
    wv, hv = struct.unpack("<HH", d[s + 6:s + 10])
    f.width, f.height, f.xscale, f.yscale = wv & 0x3fff, hv & 0x3fff, wv >> 14, hv >> 14
    p0 = s + 10
    p0_end = p0 + (tag >> 5)
    assert p0_end <= e
    io0 = BoolDecoder(d, p0, p0_end)
    walk_header(io0, f)
    n = 1 << f.log2_parts
    status = 0
    table = p0_end
    start = table + 3 * (n - 1)
    parts = [(p0, p0_end)]
    if start > e:
        return f, STATUS_BAD_PARTITIONS, parts
    for i in range(n - 1):
        size = d[table + 3 * i] | d[table + 3 * i + 1] << 8 | d[table + 3 * i + 2] << 16
        size = min(size, e - start)
        parts.append((start, start + size))
        start += size
    parts.append((start, e))
    if start >= e:
        return f, STATUS_BAD_PARTITIONS, parts
    walk_header_tail(io0, f)
    ios = [BoolDecoder(d, a, b) for a, b in parts[1:]]
    walk_frame(io0, ios, f, True)
    if io0.eof or any(io.eof for io in ios):
        status |= STATUS_INPUT_EXHAUSTED
    return f, status, parts


# ---------------------------------------------------------------- writing a frame

def write_frame(f):
    """Frame -> the payload of a `VP8 ` chunk."""
    n = 1 << f.log2_parts
    io0 = BoolEncoder()
    walk_header(io0, f)
    walk_header_tail(io0, f)
    ios = [BoolEncoder() for _ in range(n)]
    walk_frame(io0, ios, f, False)
    first = io0.finish()
    parts = [io.finish() for io in ios]
    tag = 0 | 0 << 1 | 1 << 4 | len(first) << 5
    out = bytes([tag & 255, tag >> 8 & 255, tag >> 16 & 255]) + b"\x9d\x01\x2a" + struct.pack("<HH", f.width | f.xscale << 14, f.height | f.yscale << 14)
    out += first + b"".join(struct.pack("<I", len(p))[:3] for p in parts[:-1]) + b"".join(parts)
    return out


def transcode(d, segmentation=None, **changes):
    """The file `d` written again with the same modes and coefficient levels and with header fields replaced: any attribute of Frame
    (simple, level, sharpness, use_lf_delta, lf_update, ref_delta, mode_delta, dq, base_q, colorspace, clamp, xscale, yscale, log2_parts,
    use_skip, ...).  segmentation="off" drops the segment map and data, "absolute" rewrites the per-segment values as absolute ones."""
    f, status, _ = describe(d)
    assert status == 0
    if segmentation == "off":
        f.use_segment = f.update_map = f.update_data = 0
    elif segmentation == "absolute":
        assert f.use_segment
        if not f.absolute:
            f.seg_quant = [min(max(q + f.base_q, 0), 127) for q in f.seg_quant]
            f.seg_filter = [min(max(q + f.level, 0), 63) for q in f.seg_filter]
        f.absolute = f.update_data = 1
    for k, v in changes.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    if f.use_lf_delta and (any(f.ref_delta) or any(f.mode_delta)):
        f.lf_update = 1
    return replace_payload(bytes(d), write_frame(f))


# ---------------------------------------------------------------- reconstruction

def _mul1(a):
    return ((a * 20091) >> 16) + a


def _mul2(a):
    return (a * 35468) >> 16


def idct(c):
    """16 dequantised coefficients in raster order -> the 4 x 4 residual [row][column]."""
    tmp = [0] * 16
    for i in range(4):
        a, b = c[i] + c[8 + i], c[i] - c[8 + i]
        cc, dd = _mul2(c[4 + i]) - _mul1(c[12 + i]), _mul1(c[4 + i]) + _mul2(c[12 + i])
        tmp[4 * i:4 * i + 4] = a + dd, b + cc, b - cc, a - dd
    out = np.zeros((4, 4), np.int32)
    for i in range(4):
        dc = tmp[i] + 4
        a, b = dc + tmp[8 + i], dc - tmp[8 + i]
        cc, dd = _mul2(tmp[4 + i]) - _mul1(tmp[12 + i]), _mul1(tmp[4 + i]) + _mul2(tmp[12 + i])
        out[i] = (a + dd) >> 3, (b + cc) >> 3, (b - cc) >> 3, (a - dd) >> 3
    return out


def iwht(c):
    """The 16 Y2 coefficients -> the DC of the 16 luma blocks."""
    tmp = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = c[i] + c[12 + i], c[4 + i] + c[8 + i], c[4 + i] - c[8 + i], c[i] - c[12 + i]
        tmp[i], tmp[8 + i], tmp[4 + i], tmp[12 + i] = a0 + a1, a0 - a1, a3 + a2, a3 - a2
    out = [0] * 16
    for i in range(4):
        dc = tmp[4 * i] + 3
        a0, a1, a2, a3 = dc + tmp[4 * i + 3], tmp[4 * i + 1] + tmp[4 * i + 2], tmp[4 * i + 1] - tmp[4 * i + 2], dc - tmp[4 * i + 3]
        out[4 * i:4 * i + 4] = (a0 + a1) >> 3, (a3 + a2) >> 3, (a0 - a1) >> 3, (a3 - a2) >> 3
    return out


def _i16(v):
    return ((int(v) + 32768) & 0xffff) - 32768


def dequantise(f, mb, q):
    """The levels of a macroblock -> [24][16] coefficients in raster order (int16, the Y2 block folded into the luma DCs)."""
    y1dc, y1ac, y2dc, y2ac, uvdc, uvac, _ = q
    lv = mb["levels"]
    co = [[0] * 16 for _ in range(24)]
    for b in range(24):
        dc, ac = (y1dc, y1ac) if b < 16 else (uvdc, uvac)
        for n in range(16):
            if lv[b][n]:
                co[b][ZIGZAG[n]] = _i16(lv[b][n] * (ac if n else dc))
    if not mb["i4"]:
        y2 = [0] * 16
        for n in range(16):
            if lv[24][n]:
                y2[ZIGZAG[n]] = _i16(lv[24][n] * (y2ac if n else y2dc))
        if mb["nz"][24] > 1:
            dcs = iwht(y2)
            counters["y2_ac"] += 1
        else:
            dcs = [(y2[0] + 3) >> 3] * 16
        for b in range(16):
            co[b][0] = _i16(dcs[b])
    return co


def _avg3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def _avg2(a, b):
    return (a + b + 1) >> 1


def predict4(mode, t, l):
    """t: X A B C D E F G H (the corner, 4 above, 4 above-right), l: I J K L -> 4 x 4 [row][column]."""
    X, A, B, C, D, E, F, G, H = (int(v) for v in t)
    I, J, K, L = (int(v) for v in l)
    o = np.zeros((4, 4), np.int32)

    def put(v, *xy):
        for x, y in xy:
            o[y, x] = v
    if mode == B_DC:
        o[:] = (A + B + C + D + I + J + K + L + 4) >> 3
    elif mode == B_TM:
        o[:] = np.clip(np.array([A, B, C, D])[None, :] + np.array([I, J, K, L])[:, None] - X, 0, 255)
    elif mode == B_VE:
        o[:] = [_avg3(X, A, B), _avg3(A, B, C), _avg3(B, C, D), _avg3(C, D, E)]
    elif mode == B_HE:
        o[:] = np.array([_avg3(X, I, J), _avg3(I, J, K), _avg3(J, K, L), _avg3(K, L, L)])[:, None]
    elif mode == B_RD:
        put(_avg3(J, K, L), (0, 3))
        put(_avg3(I, J, K), (1, 3), (0, 2))
        put(_avg3(X, I, J), (2, 3), (1, 2), (0, 1))
        put(_avg3(A, X, I), (3, 3), (2, 2), (1, 1), (0, 0))
        put(_avg3(B, A, X), (3, 2), (2, 1), (1, 0))
        put(_avg3(C, B, A), (3, 1), (2, 0))
        put(_avg3(D, C, B), (3, 0))
    elif mode == B_VR:
        put(_avg2(X, A), (0, 0), (1, 2))
        put(_avg2(A, B), (1, 0), (2, 2))
        put(_avg2(B, C), (2, 0), (3, 2))
        put(_avg2(C, D), (3, 0))
        put(_avg3(K, J, I), (0, 3))
        put(_avg3(J, I, X), (0, 2))
        put(_avg3(I, X, A), (0, 1), (1, 3))
        put(_avg3(X, A, B), (1, 1), (2, 3))
        put(_avg3(A, B, C), (2, 1), (3, 3))
        put(_avg3(B, C, D), (3, 1))
    elif mode == B_LD:
        put(_avg3(A, B, C), (0, 0))
        put(_avg3(B, C, D), (1, 0), (0, 1))
        put(_avg3(C, D, E), (2, 0), (1, 1), (0, 2))
        put(_avg3(D, E, F), (3, 0), (2, 1), (1, 2), (0, 3))
        put(_avg3(E, F, G), (3, 1), (2, 2), (1, 3))
        put(_avg3(F, G, H), (3, 2), (2, 3))
        put(_avg3(G, H, H), (3, 3))
    elif mode == B_VL:
        put(_avg2(A, B), (0, 0))
        put(_avg2(B, C), (1, 0), (0, 2))
        put(_avg2(C, D), (2, 0), (1, 2))
        put(_avg2(D, E), (3, 0), (2, 2))
        put(_avg3(A, B, C), (0, 1))
        put(_avg3(B, C, D), (1, 1), (0, 3))
        put(_avg3(C, D, E), (2, 1), (1, 3))
        put(_avg3(D, E, F), (3, 1), (2, 3))
        put(_avg3(E, F, G), (3, 2))
        put(_avg3(F, G, H), (3, 3))
    elif mode == B_HD:
        put(_avg2(I, X), (0, 0), (2, 1))
        put(_avg2(J, I), (0, 1), (2, 2))
        put(_avg2(K, J), (0, 2), (2, 3))
        put(_avg2(L, K), (0, 3))
        put(_avg3(A, B, C), (3, 0))
        put(_avg3(X, A, B), (2, 0))
        put(_avg3(I, X, A), (1, 0), (3, 1))
        put(_avg3(J, I, X), (1, 1), (3, 2))
        put(_avg3(K, J, I), (1, 2), (3, 3))
        put(_avg3(L, K, J), (1, 3))
    else:
        put(_avg2(I, J), (0, 0))
        put(_avg2(J, K), (2, 0), (0, 1))
        put(_avg2(K, L), (2, 1), (0, 2))
        put(_avg3(I, J, K), (1, 0))
        put(_avg3(J, K, L), (3, 0), (1, 1))
        put(_avg3(K, L, L), (3, 1), (1, 2))
        put(L, (3, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))
    return o


def predict_block(mode, W, n, mx, my):
    """A 16 x 16 or 8 x 8 prediction inside the work array W (row 0 = the row above, column 0 = the column to the left)."""
    top, left, corner = W[0, 1:n + 1].astype(np.int32), W[1:n + 1, 0].astype(np.int32), int(W[0, 0])
    sh = 4 if n == 16 else 3
    if mode == DC_PRED:
        if mx and my:
            v = (int(top.sum()) + int(left.sum()) + n) >> (sh + 1)
        elif my:
            v = (int(top.sum()) + (n >> 1)) >> sh
        elif mx:
            v = (int(left.sum()) + (n >> 1)) >> sh
        else:
            v = 128
        W[1:n + 1, 1:n + 1] = v
    elif mode == TM_PRED:
        W[1:n + 1, 1:n + 1] = np.clip(top[None, :] + left[:, None] - corner, 0, 255)
    elif mode == V_PRED:
        W[1:n + 1, 1:n + 1] = top[None, :]
    else:
        W[1:n + 1, 1:n + 1] = left[:, None]


def _work(P, mx, my, n, extra):
    """The work array of a macroblock: the samples of plane P above and to the left, with the normative borders."""
    W = np.zeros((n + 1, n + 1 + extra), np.int32)
    x0, y0 = mx * n, my * n
    W[0, 1:] = 127
    W[1:, 0] = 129
    W[0, 0] = 127
    if my:
        W[0, 1:n + 1] = P[y0 - 1, x0:x0 + n]
        W[0, 0] = P[y0 - 1, x0 - 1] if mx else 129
        if extra:
            W[0, n + 1:] = P[y0 - 1, x0 + n:x0 + n + extra] if x0 + n < P.shape[1] else P[y0 - 1, x0 + n - 1]
    if mx:
        W[1:, 0] = P[y0:y0 + n, x0 - 1]
    return W


def reconstruct(f):
    """The unfiltered planes, padded to whole macroblocks (int32 arrays with values 0 .. 255)."""
    mbw, mbh = f.mbw, f.mbh
    Y, U, V = np.zeros((16 * mbh, 16 * mbw), np.int32), np.zeros((8 * mbh, 8 * mbw), np.int32), np.zeros((8 * mbh, 8 * mbw), np.int32)
    qs = quantisers(f)
    for my in range(mbh):
        for mx in range(mbw):
            mb = f.mbs[my * mbw + mx]
            q = qs[mb["segment"]]
            for k, ix in enumerate(q[6]):
                counters["q%d" % ix] += 1
            co = dequantise(f, mb, q)
            mb["any_coeff"] = any(v for b in co for v in b)          # what switches the inner edges on in a 16x16-predicted macroblock
            assert max(abs(v) for b in co for v in b) <= 32767
            counters["max_coeff"] = max(counters["max_coeff"], max(abs(v) for b in co for v in b))
            counters["type_i4" if mb["i4"] else "type_i16"] += 1
            W = _work(Y, mx, my, 16, 4)
            if mb["i4"]:
                W[4, 17:] = W[8, 17:] = W[12, 17:] = W[0, 17:]
                for b in range(16):
                    r0, c0 = 1 + 4 * (b >> 2), 1 + 4 * (b & 3)
                    counters["bmode%d" % mb["modes"][b]] += 1
                    pred = predict4(mb["modes"][b], W[r0 - 1, c0 - 1:c0 + 8], W[r0:r0 + 4, c0 - 1])
                    W[r0:r0 + 4, c0:c0 + 4] = np.clip(pred + idct(co[b]), 0, 255)
            else:
                counters["ymode%d" % mb["ymode"]] += 1
                predict_block(mb["ymode"], W, 16, mx, my)
                for b in range(16):
                    r0, c0 = 1 + 4 * (b >> 2), 1 + 4 * (b & 3)
                    W[r0:r0 + 4, c0:c0 + 4] = np.clip(W[r0:r0 + 4, c0:c0 + 4] + idct(co[b]), 0, 255)
            Y[16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = W[1:17, 1:17]
            counters["uvmode%d" % mb["uvmode"]] += 1
            for ch, P in ((0, U), (1, V)):
                W = _work(P, mx, my, 8, 0)
                predict_block(mb["uvmode"], W, 8, mx, my)
                for b in range(4):
                    r0, c0 = 1 + 4 * (b >> 1), 1 + 4 * (b & 1)
                    W[r0:r0 + 4, c0:c0 + 4] = np.clip(W[r0:r0 + 4, c0:c0 + 4] + idct(co[16 + 4 * ch + b]), 0, 255)
                P[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = W[1:9, 1:9]
            if mb["skip"]:
                counters["skipped"] += 1
    return Y, U, V


# ---------------------------------------------------------------- loop filter

def _filter_edge(seg, kind, thresh, ithresh, hev_t):
    """seg: int32 [8, n], the samples p3 p2 p1 p0 | q0 q1 q2 q3 across an edge for n positions along it, changed in place.
    kind: 'simple', 'mb' (macroblock edge: 6 samples) or 'inner' (4 samples)."""
    p3, p2, p1, p0, q0, q1, q2, q3 = (seg[i].copy() for i in range(8))
    mask = 4 * np.abs(p0 - q0) + np.abs(p1 - q1) <= 2 * thresh + 1

    def c1(v):
        return np.clip(v, -128, 127)

    def c2(v):
        return np.clip(v, -16, 15)

    def px(v):
        return np.clip(v, 0, 255)
    a = 3 * (q0 - p0) + c1(p1 - q1)
    f2_p0, f2_q0 = px(p0 + c2((a + 3) >> 3)), px(q0 - c2((a + 4) >> 3))
    if kind == "simple":
        seg[3], seg[4] = np.where(mask, f2_p0, p0), np.where(mask, f2_q0, q0)
        return
    for u, v in ((p3, p2), (p2, p1), (p1, p0), (q3, q2), (q2, q1), (q1, q0)):
        mask &= np.abs(u - v) <= ithresh
    hev = (np.abs(p1 - p0) > hev_t) | (np.abs(q1 - q0) > hev_t)
    new = [p2, p1, np.where(hev, f2_p0, p0), np.where(hev, f2_q0, q0), q1, q2]
    if kind == "mb":
        a = c1(3 * (q0 - p0) + c1(p1 - q1))
        a1, a2, a3 = (27 * a + 63) >> 7, (18 * a + 63) >> 7, (9 * a + 63) >> 7
        other = [px(p2 + a3), px(p1 + a2), px(p0 + a1), px(q0 - a1), px(q1 - a2), px(q2 - a3)]
    else:
        a = 3 * (q0 - p0)
        a1, a2 = c2((a + 4) >> 3), c2((a + 3) >> 3)
        a3 = (a1 + 1) >> 1
        other = [p2, px(p1 + a3), px(p0 + a2), px(q0 - a1), px(q1 - a3), q2]
    for i in range(6):
        seg[1 + i] = np.where(mask, np.where(hev, new[i], other[i]), seg[1 + i])


def loop_filter(f, planes):
    """The planes of reconstruct(), filtered in place in macroblock raster order."""
    Y, U, V = planes
    mbw, mbh = f.mbw, f.mbh
    fs = filter_strengths(f)
    ftype = 0 if f.level == 0 else 1 if f.simple else 2
    if ftype == 0:
        counters["filter_none"] += 1
        return
    counters["filter_simple" if ftype == 1 else "filter_normal"] += 1

    def vertical_edge(P, x, y0, n, *a):      # an edge between columns x - 1 and x, n rows from y0
        seg = P[y0:y0 + n, x - 4:x + 4].T.copy()
        _filter_edge(seg, *a)
        P[y0:y0 + n, x - 4:x + 4] = seg.T

    def horizontal_edge(P, y, x0, n, *a):
        seg = P[y - 4:y + 4, x0:x0 + n].copy()
        _filter_edge(seg, *a)
        P[y - 4:y + 4, x0:x0 + n] = seg

    for my in range(mbh):
        for mx in range(mbw):
            mb = f.mbs[my * mbw + mx]
            limit, il, hev = fs[mb["segment"]][mb["i4"]]
            inner = bool(mb["i4"]) or mb["any_coeff"]
            if limit == 0:
                counters["mb_unfiltered"] += 1
                continue
            counters["inner_on" if inner else "inner_off"] += 1
            counters["hev%d" % hev] += 1
            x0, y0 = 16 * mx, 16 * my
            if ftype == 1:
                if mx:
                    vertical_edge(Y, x0, y0, 16, "simple", limit + 4, 0, 0)
                if inner:
                    for k in (4, 8, 12):
                        vertical_edge(Y, x0 + k, y0, 16, "simple", limit, 0, 0)
                if my:
                    horizontal_edge(Y, y0, x0, 16, "simple", limit + 4, 0, 0)
                if inner:
                    for k in (4, 8, 12):
                        horizontal_edge(Y, y0 + k, x0, 16, "simple", limit, 0, 0)
                continue
            for P, n in ((Y, 16), (U, 8), (V, 8)):
                x0, y0 = n * mx, n * my
                inners = (4, 8, 12) if n == 16 else (4,)
                if mx:
                    vertical_edge(P, x0, y0, n, "mb", limit + 4, il, hev)
                if inner:
                    for k in inners:
                        vertical_edge(P, x0 + k, y0, n, "inner", limit, il, hev)
                if my:
                    horizontal_edge(P, y0, x0, n, "mb", limit + 4, il, hev)
                if inner:
                    for k in inners:
                        horizontal_edge(P, y0 + k, x0, n, "inner", limit, il, hev)


# ---------------------------------------------------------------- upsampling and colour

def upsample(C, w, h):
    """A chroma plane [ceil(h / 2), ceil(w / 2)] -> [h, w] by libwebp's fancy upsampler: per output sample the nearest chroma sample N, its
    horizontal neighbour H, its vertical neighbour V and the diagonal one D (neighbours clamped at the borders) give
    (((N + H + V + D + 8 + 2 * (H + V)) >> 3) + N) >> 1 — two roundings, not (9 N + 3 H + 3 V + D + 8) >> 4."""
    C = C.astype(np.int32)
    ch, cw = C.shape
    r, c = np.arange(h), np.arange(w)
    nr, nc = np.where(r & 1, (r - 1) >> 1, r >> 1), np.where(c & 1, (c - 1) >> 1, c >> 1)
    fr, fc = np.clip(np.where(r & 1, nr + 1, nr - 1), 0, ch - 1), np.clip(np.where(c & 1, nc + 1, nc - 1), 0, cw - 1)
    N, H, V, D = C[nr][:, nc], C[nr][:, fc], C[fr][:, nc], C[fr][:, fc]
    return (((N + H + V + D + 8 + 2 * (H + V)) >> 3) + N) >> 1


def yuv_to_bgr(Y, U, V):
    """Full-size planes -> uint8 [h, w, 3] BGR by libwebp's 14-bit fixed point."""
    y, u, v = (p.astype(np.int32) for p in (Y, U, V))
    yy = (y * 19077) >> 8

    def clip(x):
        return np.clip(x >> 6, 0, 255).astype(np.uint8)
    r = clip(yy + ((v * 26149) >> 8) - 14234)
    g = clip(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708)
    b = clip(yy + ((u * 33050) >> 8) - 17685)
    return np.stack([b, g, r], -1)


def decode_planes(d):
    """-> (Frame, unfiltered padded planes, filtered padded planes, status)"""
    f, status, _ = describe(d)
    if status:
        return f, None, None, status
    recon = reconstruct(f)
    done = tuple(p.copy() for p in recon)
    loop_filter(f, done)
    return f, recon, done, 0


def decode_stages(d):
    f, _, done, status = decode_planes(d)
    w, h = f.width, f.height
    if status:
        return np.zeros((h, w, 3), np.uint8), None, status
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    Y, U, V = done[0][:h, :w], done[1][:ch, :cw], done[2][:ch, :cw]
    bgr = yuv_to_bgr(Y, upsample(U, w, h), upsample(V, w, h))
    return bgr, tuple(p.astype(np.uint8) for p in (Y, U, V)), 0
