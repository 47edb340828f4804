"""The rule book of lossless WebP (the VP8L bit stream) in plain Python / NumPy, and a small hand assembler for the paths a stock writer does not take.

decode_stages(file) follows the same steps, in the same order, as csrc/webp_decode.hip and predicts its status word: decoding stops at the first
fault and reports that fault's bit, except that a fault met after a bit past the end of the stream has been consumed is reported as
ST_INPUT_EXHAUSTED (the zeros fed past the end are not the file's), and so is a decode that ends without a fault but has consumed such a bit.
COUNTERS notes every path a decode took (tools/make_golden_webp.py asserts the fixture set reaches them all).
"""
import struct
from collections import Counter

import numpy as np

(ST_INPUT_EXHAUSTED, ST_BAD_TRANSFORM, ST_BAD_CACHE_BITS, ST_BAD_CODE_LENGTHS, ST_NO_CODE, ST_DISTANCE_TOO_FAR, ST_COPY_PAST_END,
 ST_TABLE_SPACE) = (1 << i for i in range(8))

CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
K = bytes.fromhex("1807171928062729161a262a3805373915 1b363a252b48044749141c353b464a"
                  "242c58454b343c035759131d565a232d444c555b333d68026769121e666a222e"
                  "545c434d656b323e78017779535d111f646c424e767a212f757b313f636d525e"
                  "00747c414f1020626e30737d515f40727e616f50717f6070".replace(" ", ""))
assert len(K) == 120
HASH = 0x1e35a7bd
MAX_LENGTH = 4096
COUNTERS = Counter()


class Fail(Exception):
    def __init__(self, bit):
        Exception.__init__(self, "status 0x%x" % bit)
        self.bit = bit


class Bits:
    """LSB-first reader; past the end it feeds zeros and remembers that it did."""

    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.n = 8 * len(data)
        self.p = 0

    def bits(self, k):
        r = (self.v >> self.p) & ((1 << k) - 1)
        self.p += k
        return r

    def exhausted(self):
        return self.p > self.n

    def fail(self, bit):
        return Fail(ST_INPUT_EXHAUSTED if self.exhausted() else bit)


def subsample(n, b):
    return (n + (1 << b) - 1) >> b


# ------------------------------------------------------------------ prefix codes

class Code:
    """A canonical code: decode walks the lengths as the device does."""

    def __init__(self, lengths):
        self.cnt = [0] * 16
        for l in lengths:
            self.cnt[l] += 1
        self.cnt[0] = 0
        self.sorted = [s for l in range(1, 16) for s, ls in enumerate(lengths) if ls == l]
        self.single = self.sorted[0] if len(self.sorted) == 1 else -1

    def complete(self):
        if self.single >= 0:
            return True
        left = 1
        for l in range(1, 16):
            left = 2 * left - self.cnt[l]
            if left < 0:
                return False
        return left == 0 and len(self.sorted) > 0

    def read(self, br):
        if self.single >= 0:
            return self.single
        code = first = index = 0
        for l in range(1, 16):
            code |= br.bits(1)
            c = self.cnt[l]
            if code - first < c:
                return self.sorted[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise br.fail(ST_NO_CODE)


def read_code(br, alphabet):
    lengths = [0] * alphabet
    if br.bits(1):
        k = br.bits(1) + 1
        first8 = br.bits(1)
        syms = [br.bits(8 if first8 else 1)]
        if k == 2:
            syms.append(br.bits(8))
        COUNTERS["simple%d_%dbit" % (k, 8 if first8 else 1)] += 1
        for s in syms:
            if s >= alphabet:
                raise br.fail(ST_BAD_CODE_LENGTHS)
            lengths[s] = 1
    else:
        n = 4 + br.bits(4)
        cl = [0] * 19
        for i in range(n):
            cl[CL_ORDER[i]] = br.bits(3)
        clc = Code(cl)
        if not clc.complete():
            raise br.fail(ST_BAD_CODE_LENGTHS)
        if br.bits(1):
            max_symbol = 2 + br.bits(2 + 2 * br.bits(3))
            if max_symbol > alphabet:
                raise br.fail(ST_BAD_CODE_LENGTHS)
            COUNTERS["normal_max_symbol"] += 1
        else:
            max_symbol = alphabet
            COUNTERS["normal_plain"] += 1
        s, prev = 0, 8
        any_nonzero = False
        while s < alphabet and max_symbol > 0:
            max_symbol -= 1
            t = clc.read(br)
            if t < 16:
                lengths[s] = t
                s += 1
                if t:
                    prev = t
                    any_nonzero = True
            else:
                if t == 16:
                    rep, v = 3 + br.bits(2), prev
                    COUNTERS["token16"] += 1
                    if not any_nonzero:
                        COUNTERS["token16_first"] += 1
                    any_nonzero = True
                elif t == 17:
                    rep, v = 3 + br.bits(3), 0
                    COUNTERS["token17"] += 1
                else:
                    rep, v = 11 + br.bits(7), 0
                    COUNTERS["token18"] += 1
                if s + rep > alphabet:
                    raise br.fail(ST_BAD_CODE_LENGTHS)
                lengths[s:s + rep] = [v] * rep
                s += rep
    code = Code(lengths)
    if not code.complete():
        raise br.fail(ST_BAD_CODE_LENGTHS)
    if br.exhausted():
        raise br.fail(ST_INPUT_EXHAUSTED)
    return code


def prefix_value(br, p):
    if p < 4:
        return p + 1
    e = (p - 2) >> 1
    return ((2 + (p & 1)) << e) + br.bits(e) + 1


def plane_distance(dc, w):
    if dc > 120:
        COUNTERS["far_distance"] += 1
        return dc - 120
    k = K[dc - 1]
    d = (k >> 4) * w + 8 - (k & 15)
    COUNTERS["plane_code"] += 1
    if d < 1:
        COUNTERS["plane_clamp"] += 1
        d = 1
    return d


# ------------------------------------------------------------------ an entropy-coded image

def read_image(br, w, h, main):
    """-> the w * h pixels (a list of ARGB ints)."""
    cache_bits = 0
    if br.bits(1):
        cache_bits = br.bits(4)
        if cache_bits < 1 or cache_bits > 11:
            raise br.fail(ST_BAD_CACHE_BITS)
        COUNTERS["cache_bits_%d" % cache_bits] += 1
    csize = (1 << cache_bits) if cache_bits else 0
    groups, pb, meta, mw = 1, 0, None, 0
    if main and br.bits(1):
        pb = br.bits(3) + 2
        mw = subsample(w, pb)
        meta = read_image(br, mw, subsample(h, pb), False)
        groups = max((m >> 8) & 0xffff for m in meta) + 1
        COUNTERS["meta_groups_%s" % ("1" if groups == 1 else "many")] += 1
    codes = []
    for g in range(groups):
        codes.append([read_code(br, a) for a in (280 + csize, 256, 256, 256, 40)])
    n = w * h
    out = [0] * n
    cache = [0] * csize
    p = 0
    while p < n:
        g = codes[(meta[(p // w >> pb) * mw + (p % w >> pb)] >> 8) & 0xffff] if meta else codes[0]
        s = g[0].read(br)
        if s < 256:
            r = g[1].read(br)
            b = g[2].read(br)
            a = g[3].read(br)
            out[p] = a << 24 | r << 16 | s << 8 | b
            if csize:
                cache[(HASH * out[p] & 0xffffffff) >> (32 - cache_bits)] = out[p]
            p += 1
        elif s < 280:
            L = prefix_value(br, s - 256)
            D = plane_distance(prefix_value(br, g[4].read(br)), w)
            if br.exhausted():
                raise br.fail(ST_INPUT_EXHAUSTED)
            if D > p:
                raise br.fail(ST_DISTANCE_TOO_FAR)
            if L > n - p:
                raise br.fail(ST_COPY_PAST_END)
            if main:
                COUNTERS["copy"] += 1
                if D == 1:
                    COUNTERS["copy_distance_1"] += 1
                if D < L:
                    COUNTERS["copy_overlap"] += 1
                if p % w + L > w:
                    COUNTERS["copy_across_row"] += 1
                if L == MAX_LENGTH:
                    COUNTERS["copy_4096"] += 1
                if D > 8192:
                    COUNTERS["copy_beyond_8192"] += 1                   # further back than the device keeps in its LDS ring
            for i in range(L):
                v = out[p + i] = out[p + i - D]
                if csize:
                    cache[(HASH * v & 0xffffffff) >> (32 - cache_bits)] = v
            p += L
        else:
            out[p] = cache[s - 280]
            COUNTERS["cache_hit"] += 1
            cache[(HASH * out[p] & 0xffffffff) >> (32 - cache_bits)] = out[p]
            p += 1
        if br.exhausted():
            raise br.fail(ST_INPUT_EXHAUSTED)
    return out


# ------------------------------------------------------------------ inverse transforms

def _avg(a, b):
    return (((a ^ b) & 0xfefefefe) >> 1) + (a & b)


def _ch(v):
    return (v >> 24, v >> 16 & 255, v >> 8 & 255, v & 255)


def _pack(c):
    return c[0] << 24 | c[1] << 16 | c[2] << 8 | c[3]


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _trunc_half(v):
    return -((-v) >> 1) if v < 0 else v >> 1


def predict(mode, L, T, TL, TR):
    if mode == 0 or mode > 13:
        return 0xff000000
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    l, t, tl = _ch(L), _ch(T), _ch(TL)
    if mode == 11:
        return L if sum(abs(a - c) for a, c in zip(t, tl)) < sum(abs(a - c) for a, c in zip(l, tl)) else T
    if mode == 12:
        return _pack([_clip(a + b - c) for a, b, c in zip(l, t, tl)])
    av = _ch(_avg(L, T))
    return _pack([_clip(a + _trunc_half(a - c)) for a, c in zip(av, tl)])


def _add(a, b):
    return ((a & 0xff00ff00) + (b & 0xff00ff00) & 0xff00ff00) | ((a & 0x00ff00ff) + (b & 0x00ff00ff) & 0x00ff00ff)


def inverse_predictor(px, w, h, b, blocks):
    bw = subsample(w, b)
    out = list(px)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pred = 0xff000000 if x == 0 else out[i - 1]
            elif x == 0:
                pred = out[i - w]
            else:
                mode = blocks[(y >> b) * bw + (x >> b)] >> 8 & 15
                COUNTERS["pred_mode_%d" % mode] += 1
                pred = predict(mode, out[i - 1], out[i - w], out[i - w - 1], out[i - w + 1])      # x == w - 1: the next word is this row's first pixel
            out[i] = _add(out[i], pred)
    return out


def _s8(v):
    return v - 256 if v > 127 else v


def inverse_cross(px, w, h, b, blocks):
    bw = subsample(w, b)
    out = []
    for i, v in enumerate(px):
        m = blocks[(i // w >> b) * bw + (i % w >> b)]
        g2r, g2b, r2b = _s8(m & 255), _s8(m >> 8 & 255), _s8(m >> 16 & 255)
        g = _s8(v >> 8 & 255)
        r = ((v >> 16 & 255) + ((g2r * g) >> 5)) & 255
        bl = ((v & 255) + ((g2b * g) >> 5)) & 255
        bl = (bl + ((r2b * _s8(r)) >> 5)) & 255
        out.append((v & 0xff00ff00) | r << 16 | bl)
    return out


def inverse_green(px):
    out = []
    for v in px:
        g = v >> 8 & 255
        out.append((v & 0xff00ff00) | ((v >> 16 & 255) + g & 255) << 16 | ((v & 255) + g & 255))
    return out


def inverse_palette(px, w, h, wb, n, palette):
    cw = subsample(w, wb)
    per, bits = 1 << wb, 8 >> wb
    out = []
    for y in range(h):
        for x in range(w):
            idx = (px[y * cw + (x >> wb)] >> 8 & 255) >> ((x & (per - 1)) * bits) & ((1 << bits) - 1)
            if idx >= n:
                COUNTERS["index_past_palette"] += 1
            out.append(palette[idx] if idx < n else 0)
    COUNTERS["pack_%d" % per] += 1
    return out


# ------------------------------------------------------------------ the container and the whole file

def walk(d):
    """-> (VP8L payload, width, height) of a file the host side accepts (maf-yolo_amd/webp.py parse does the checking)."""
    assert d[:4] == b"RIFF" and d[8:12] == b"WEBP"
    p = 12
    while p + 8 <= len(d):
        cc, n = d[p:p + 4], struct.unpack("<I", d[p + 4:p + 8])[0]
        if cc == b"VP8L":
            pay = d[p + 8:p + 8 + n]
            v = int.from_bytes(pay[1:5], "little")
            return pay, (v & 0x3fff) + 1, (v >> 14 & 0x3fff) + 1
        p += 8 + n + (n & 1)
    raise ValueError("no VP8L chunk")


def decode_stages(d):
    """-> (bgr uint8 [h, w, 3], argb uint32 [h, coded width] before the inverse transforms, status).  A non-zero status comes with an
    all-zero frame and an all-zero argb of the full width."""
    pay, w, h = walk(d)
    br = Bits(pay[5:])
    try:
        cw = w
        transforms, seen = [], set()
        while br.bits(1):
            t = br.bits(2)
            if t in seen:
                raise br.fail(ST_BAD_TRANSFORM)
            seen.add(t)
            if t < 2:
                b = br.bits(3) + 2
                transforms.append((t, b, cw, read_image(br, subsample(cw, b), subsample(h, b), False)))
            elif t == 2:
                transforms.append((t, 0, cw, None))
            else:
                n = br.bits(8) + 1
                pal = read_image(br, n, 1, False)
                for i in range(1, n):
                    pal[i] = _add(pal[i], pal[i - 1])
                wb = 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0
                transforms.append((t, wb, cw, (n, pal)))
                cw = subsample(cw, wb)
            if br.exhausted():
                raise br.fail(ST_INPUT_EXHAUSTED)
        COUNTERS["order_" + "".join(str(t[0]) for t in transforms)] += 1
        px = read_image(br, cw, h, True)
        if br.exhausted():
            raise br.fail(ST_INPUT_EXHAUSTED)
    except Fail as f:
        return np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint32), f.bit
    argb = np.array(px, np.uint32).reshape(h, cw)
    for t, b, tw, data in reversed(transforms):
        if t == 0:
            px = inverse_predictor(px, tw, h, b, data)
        elif t == 1:
            px = inverse_cross(px, tw, h, b, data)
        elif t == 2:
            px = inverse_green(px)
        else:
            px = inverse_palette(px, tw, h, b, data[0], data[1])
    out = np.array(px, np.uint32).reshape(h, w)
    bgr = np.stack([out & 255, out >> 8 & 255, out >> 16 & 255], -1).astype(np.uint8)
    return bgr, argb, 0


# ------------------------------------------------------------------ the hand assembler

class BitWriter:
    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, value, k):
        assert 0 <= value < (1 << k) or k == 0
        self.v |= value << self.n
        self.n += k

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """{symbol: (code, length)} of a canonical code; the first stream bit is the most significant code bit."""
    code, out = 0, {}
    for l in range(1, 16):
        for s, ls in enumerate(lengths):
            if ls == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def put_symbol(bw, table, s):
    if len(table) == 1:
        assert s in table
        return                                                  # a one-symbol code consumes no bits
    code, l = table[s]
    for i in range(l - 1, -1, -1):
        bw.put(code >> i & 1, 1)


def complete_lengths(used, alphabet):
    """Lengths of a complete code over the symbols `used` (a single symbol: length 1, which the reader takes as a zero-bit code)."""
    used = sorted(set(used))
    lengths = [0] * alphabet
    n = len(used)
    if n == 1:
        lengths[used[0]] = 1
        return lengths
    k = (n - 1).bit_length()
    short = (1 << k) - n
    for i, s in enumerate(used):
        lengths[s] = k - 1 if i < short else k
    return lengths


def put_simple(bw, symbols, first8=None):
    """A simple code of one or two symbols; first8: whether the first symbol takes 8 bits (default: only when it needs them)."""
    bw.put(1, 1)
    bw.put(len(symbols) - 1, 1)
    if first8 is None:
        first8 = symbols[0] > 1
    bw.put(int(first8), 1)
    bw.put(symbols[0], 8 if first8 else 1)
    if len(symbols) == 2:
        bw.put(symbols[1], 8)
    return {s: (i, 1) for i, s in enumerate(sorted(symbols))} if len(symbols) == 2 else {symbols[0]: (0, 0)}


def length_tokens(lengths, runs=True, trim=False):
    """The code-length tokens [(token, extra value)] of `lengths` (trim: trailing zeros left out, which only a written token count allows);
    with runs, tokens 16 / 17 / 18 where they fit."""
    end = len(lengths)
    while trim and end and lengths[end - 1] == 0:
        end -= 1
    toks, i, prev = [], 0, 8
    while i < end:
        v = lengths[i]
        run = 1
        while i + run < end and lengths[i + run] == v:
            run += 1
        if runs and v == 0 and run >= 11:
            r = min(run, 138)
            toks.append((18, r - 11))
        elif runs and v == 0 and run >= 3:
            r = min(run, 10)
            toks.append((17, r - 3))
        elif runs and v and v == prev and run >= 3:
            r = min(run, 6)
            toks.append((16, r - 3))
        else:
            r = 1
            toks.append((v, 0))
        if v:
            prev = v
        i += r
    return toks


def put_normal(bw, lengths, tokens=None, max_symbol=False, cl_lengths=None, runs=True):
    """A normal code with the given lengths (or an explicit token list).  max_symbol: write the token count; cl_lengths: force the lengths of the
    code-length code.  -> the canonical table of `lengths`."""
    toks = length_tokens(lengths, runs, max_symbol is not False) if tokens is None else tokens
    if cl_lengths is None:
        cl_lengths = complete_lengths([t for t, _ in toks], 19)
    bw.put(0, 1)
    n = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_lengths[s]) + 1)
    bw.put(n - 4, 4)
    for i in range(n):
        bw.put(cl_lengths[CL_ORDER[i]], 3)
    if max_symbol is False:
        bw.put(0, 1)
    else:
        count = len(toks) if max_symbol is True else max_symbol
        nb = max(2, (max(count - 2, 0)).bit_length())
        nb += nb & 1
        bw.put(1, 1)
        bw.put((nb - 2) // 2, 3)
        bw.put(count - 2, nb)
    cl = canonical(cl_lengths)
    for t, e in toks:
        put_symbol(bw, cl, t)
        if t >= 16:
            bw.put(e, (2, 3, 7)[t - 16])
    return canonical(lengths)


def prefix_encode(v):
    """A length or distance code value (>= 1) -> (prefix symbol, extra bits, their count)."""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    hb = d.bit_length() - 1
    e = hb - 1
    return 2 * hb + (d >> e & 1), d & ((1 << e) - 1), e


def put_image(bw, ops, main, cache_bits=None, meta=None, code_style="normal", override=None):
    """An entropy-coded image from `ops`: ("lit", argb), ("copy", length, distance code) or ("cache", index).  One code group, the codes
    complete over the symbols used.  meta = (pb, the entropy image's pixels): every group gets the same codes.  override = {0 .. 4: f(bw) ->
    table} writes that code of every group with f instead (the malformed cases)."""
    if cache_bits is None:
        bw.put(0, 1)
        csize = 0
    else:
        bw.put(1, 1)
        bw.put(cache_bits, 4)
        csize = 1 << cache_bits
    groups = 1
    if main:
        if meta is None:
            bw.put(0, 1)
        else:
            bw.put(1, 1)
            bw.put(meta[0] - 2, 3)
            put_image(bw, [("lit", v) for v in meta[1]], False)
            groups = max(v >> 8 & 0xffff for v in meta[1]) + 1
    used = [set(), set(), set(), set(), set()]
    for op in ops:
        if op[0] == "lit":
            v = op[1]
            used[0].add(v >> 8 & 255)
            used[1].add(v >> 16 & 255)
            used[2].add(v & 255)
            used[3].add(v >> 24)
        elif op[0] == "copy":
            used[0].add(256 + prefix_encode(op[1])[0])
            used[4].add(prefix_encode(op[2])[0])
        else:
            used[0].add(280 + op[1])
    for u in used:
        if not u:
            u.add(0)
    alph = (280 + csize, 256, 256, 256, 40)
    for g in range(groups):
        tables = []
        for k, (u, a) in enumerate(zip(used, alph)):
            u = sorted(u)
            if override and k in override:
                tables.append(override[k](bw))
            elif code_style == "simple" and len(u) <= 2 and all(s < 256 for s in u):
                tables.append(put_simple(bw, u))
            else:
                tables.append(put_normal(bw, complete_lengths(u, a)))
    for op in ops:
        if op[0] == "lit":
            v = op[1]
            put_symbol(bw, tables[0], v >> 8 & 255)
            put_symbol(bw, tables[1], v >> 16 & 255)
            put_symbol(bw, tables[2], v & 255)
            put_symbol(bw, tables[3], v >> 24)
        elif op[0] == "copy":
            s, x, e = prefix_encode(op[1])
            put_symbol(bw, tables[0], 256 + s)
            bw.put(x, e)
            s, x, e = prefix_encode(op[2])
            put_symbol(bw, tables[4], s)
            bw.put(x, e)
        else:
            put_symbol(bw, tables[0], 280 + op[1])


def hand_payload(w, h, transforms=(), ops=None, cache_bits=None, meta=None, alpha=0, version=0, code_style="normal", override=None):
    """A VP8L payload.  transforms, in reading order: ("pred", b, block pixels), ("cross", b, block pixels), ("green",), ("palette", colours
    as stored, before the cumulative addition).  ops: the main image (default: every pixel the literal 0xff000000 + its index)."""
    bw = BitWriter()
    bw.put(0x2f, 8)
    bw.put(w - 1, 14)
    bw.put(h - 1, 14)
    bw.put(alpha, 1)
    bw.put(version, 3)
    cw = w
    for t in transforms:
        bw.put(1, 1)
        bw.put({"pred": 0, "cross": 1, "green": 2, "palette": 3}[t[0]], 2)
        if t[0] in ("pred", "cross"):
            bw.put(t[1] - 2, 3)
            assert len(t[2]) == subsample(cw, t[1]) * subsample(h, t[1])
            put_image(bw, [("lit", v) for v in t[2]], False)
        elif t[0] == "palette":
            n = len(t[1])
            bw.put(n - 1, 8)
            put_image(bw, [("lit", v) for v in t[1]], False)
            cw = subsample(cw, 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0)
    bw.put(0, 1)
    if ops is None:
        ops = [("lit", 0xff000000 + (i * 0x010305 & 0xffffff)) for i in range(cw * h)]
    put_image(bw, ops, True, cache_bits, meta, code_style, override)
    return bw.bytes()


def chunk(cc, payload):
    return cc + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)


def riff(payload, extended=None, before=(), after=()):
    """A RIFF / WEBP file around a VP8L payload; extended = (width, height[, flags]) adds a VP8X chunk in front, `before` / `after` are
    (fourcc, bytes) chunks around the VP8L chunk."""
    body = b""
    if extended is not None:
        w, h = extended[:2]
        flags = extended[2] if len(extended) > 2 else 0
        body += chunk(b"VP8X", bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))
    for cc, p in before:
        body += chunk(cc, p)
    body += chunk(b"VP8L", payload)
    for cc, p in after:
        body += chunk(cc, p)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body
