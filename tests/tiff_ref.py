"""The TIFF rule book in numpy, and a hand assembler that writes a TIFF file from pixels.  No GPU, no Pillow.

What maf-yolo_amd/tiff.py and csrc/tiff_decode.hip compute, restated serially (checked against Pillow / libtiff by tools/make_golden_tiff.py and
tests/test_tiff_host.py):
  * read_ifd(d)        the first IFD of a classic TIFF file in either byte order -> {tag: [values]};
  * lzw_decode         MSB-first codes of 9 to 12 bits; Clear 256, EOI 257, first free entry 258; the code after a Clear adds no entry, every
                       later one adds exactly one; the width grows when the next free entry exceeds 2^width - 2; a code equal to the next free
                       entry is KwKwK; decoding stops once `total` bytes are out.  A code above the next free entry (or above 255 right behind
                       a Clear) is ST_LZW_BAD_CODE, a table pushed past 4095 entries ST_LZW_TABLE_FULL, bits that run out or an EOI in front of
                       the last byte ST_INPUT_EXHAUSTED; the rest of the strip is zero;
  * packbits_decode    header n in 0 .. 127: n + 1 literal bytes; -127 .. -1: the next byte 1 - n times; -128: nothing.  A literal or a run
                       byte beyond the strip is ST_PACKBITS_OVERRUN, a strip that ends early ST_INPUT_EXHAUSTED;
  * deflate_decode     a zlib stream per strip: tests/png_ref.py's inflate (the one the device runs), its status bits shifted left by 8,
                       TOO_MANY_BYTES dropped (decoding stops once the rows are full);
  * decode_stages(d)   -> (BGR uint8 [h, w, 3], the decompressed rows, the status word): strips, predictor 2 (a running sum mod 256 per row and
                       channel), then 1 bit -> 0 / 255, 4 bit -> v * 17, WhiteIsZero inverted, palette ColorMap[v] >> 8, gray replicated, RGB
                       reversed.
The assembler: pack(samples, bits) packs rows MSB first, padded to whole bytes; assemble(rows, ...) writes the file in either byte order with any
strip split, SHORT or LONG tags (values of up to 4 bytes inline, longer ones at an offset), its own LZW / PackBits encoders plus zlib, and takes
ready-made strip streams and extra or overriding tags for the cases no writer produces.
"""
import struct
import zlib

import numpy as np

import png_ref

ST_INPUT_EXHAUSTED, ST_LZW_BAD_CODE, ST_LZW_TABLE_FULL, ST_PACKBITS_OVERRUN = 1, 2, 4, 8
ST_INFLATE_SHIFT = 8
NONE, LZW, ADOBE_DEFLATE, DEFLATE, PACKBITS = 1, 5, 8, 32946, 32773
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
TYPE_CODE = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 13: "I"}
BYTE, SHORT, LONG = 1, 3, 4


# ---------------------------------------------------------------- reading

def read_ifd(d):
    """-> (byte order, {tag: [values]}) of the first IFD; only integer field types are read."""
    bo = {b"II*\0": "<", b"MM\0*": ">"}[bytes(d[:4])]
    at, = struct.unpack(bo + "I", d[4:8])
    n, = struct.unpack(bo + "H", d[at:at + 2])
    tags = {}
    for i in range(n):
        e = at + 2 + 12 * i
        tag, typ, cnt = struct.unpack(bo + "HHI", d[e:e + 8])
        if typ not in TYPE_CODE:
            continue
        size = cnt * TYPE_SIZE[typ]
        where = e + 8 if size <= 4 else struct.unpack(bo + "I", d[e + 8:e + 12])[0]
        tags.setdefault(tag, list(struct.unpack(bo + "%d%s" % (cnt, TYPE_CODE[typ]), d[where:where + size])))
    return bo, tags


def lzw_decode(buf, total):
    """One LZW strip -> (uint8 [total], status)."""
    out = bytearray()
    st = 0
    nbits = len(buf) * 8
    acc = int.from_bytes(bytes(buf), "big")
    pos, width, free, old = 0, 9, 258, None
    table = {}
    while len(out) < total:
        if pos + width > nbits:
            st |= ST_INPUT_EXHAUSTED
            break
        code = (acc >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        if code == 256:
            width, free, old = 9, 258, None
            table = {}
            continue
        if code == 257:
            st |= ST_INPUT_EXHAUSTED
            break
        if old is None:                                          # the code behind a Clear: a literal, and no entry
            if code > 257:
                st |= ST_LZW_BAD_CODE
                break
            old = bytes([code])
            out += old
            continue
        if code < 256:
            s = bytes([code])
        elif code < free:
            s = table[code]
        elif code == free:
            s = old + old[:1]                                    # KwKwK
        else:
            st |= ST_LZW_BAD_CODE
            break
        if free > 4095:
            st |= ST_LZW_TABLE_FULL
            break
        table[free] = old + s[:1]
        free += 1
        if free > (1 << width) - 2 and width < 12:
            width += 1
        out += s
        old = s
    out = bytes(out[:total])
    return np.frombuffer(out + bytes(total - len(out)), np.uint8), st


def packbits_decode(buf, total):
    out = bytearray()
    st = 0
    s, end = 0, len(buf)
    while len(out) < total and s < end and not st:
        n = buf[s] - 256 if buf[s] > 127 else buf[s]
        s += 1
        if n >= 0:
            take = min(n + 1, total - len(out))
            have = min(take, end - s)
            out += bytes(buf[s:s + have])
            s += n + 1
            if have < take:
                st |= ST_PACKBITS_OVERRUN
        elif n != -128:
            if s >= end:
                st |= ST_PACKBITS_OVERRUN
                break
            out += bytes([buf[s]]) * min(1 - n, total - len(out))
            s += 1
    if len(out) < total and not st:
        st |= ST_INPUT_EXHAUSTED
    return np.frombuffer(bytes(out) + bytes(total - len(out)), np.uint8), st


def deflate_decode(buf, total):
    got, st = png_ref.inflate(bytes(buf), total, begin=2)
    got = np.asarray(got, np.uint8)[:total]
    got = np.concatenate([got, np.zeros(total - len(got), np.uint8)])
    return got, (st & ~png_ref.ST_TOO_MANY_BYTES) << ST_INFLATE_SHIFT


def raw_decode(buf, total):
    have = min(total, len(buf))
    return np.frombuffer(bytes(buf[:have]) + bytes(total - have), np.uint8), 0 if have == total else ST_INPUT_EXHAUSTED


DECODERS = {NONE: raw_decode, LZW: lzw_decode, ADOBE_DEFLATE: deflate_decode, DEFLATE: deflate_decode, PACKBITS: packbits_decode}


def convert(rows, w, h, bits, spp, photometric, colormap=None):
    """Unpredicted rows uint8 [h, row_bytes] -> BGR uint8 [h, w, 3]."""
    if bits == 8:
        s = rows[:, :w * spp].reshape(h, w, spp).astype(np.int32)
    else:
        per = 8 // bits
        shifts = np.arange(per - 1, -1, -1) * bits
        s = ((rows[:, :, None] >> shifts) & ((1 << bits) - 1)).reshape(h, -1)[:, :w, None].astype(np.int32)
    if photometric == 2:
        return np.ascontiguousarray(s[:, :, ::-1].astype(np.uint8))
    if photometric == 3:
        cm = np.asarray(colormap, np.int64).reshape(3, 1 << bits) >> 8
        return np.ascontiguousarray(np.stack([cm[2][s[:, :, 0]], cm[1][s[:, :, 0]], cm[0][s[:, :, 0]]], -1).astype(np.uint8))
    v = s[:, :, 0] * (255 // ((1 << bits) - 1))
    if photometric == 0:
        v = 255 - v
    return np.ascontiguousarray(np.repeat(v[:, :, None], 3, axis=2).astype(np.uint8))


def decode_stages(d):
    """One supported file -> (BGR, rows uint8 [h, row_bytes] before the predictor is undone, status)."""
    bo, t = read_ifd(d)
    w, h = t[256][0], t[257][0]
    bits, spp, photometric = t.get(258, [1])[0], t.get(277, [1])[0], t[262][0]
    comp, predictor = t.get(259, [1])[0], t.get(317, [1])[0]
    rps = min(t.get(278, [h])[0], h)
    rb = (w * spp * bits + 7) // 8
    rows = np.zeros((h, rb), np.uint8)
    st = 0
    for j in range(-(-h // rps)):
        y0 = j * rps
        n = min(rps, h - y0)
        got, s = DECODERS[comp](d[t[273][j]:t[273][j] + t[279][j]], n * rb)
        rows[y0:y0 + n] = got.reshape(n, rb)
        st |= s
    und = rows
    if predictor == 2:
        und = (np.cumsum(rows.reshape(h, w, spp).astype(np.int64), axis=1) & 255).astype(np.uint8).reshape(h, rb)
    return convert(und, w, h, bits, spp, photometric, t.get(320)), rows, st


def decode(d):
    bgr, _, st = decode_stages(d)
    if st:
        raise ValueError("tiff_ref: status 0x%x" % st)
    return bgr


# ---------------------------------------------------------------- writing

def lzw_width(m):
    """The width of the m-th code behind a Clear (m = 0: the code that adds no entry)."""
    return 9 + (m >= 254) + (m >= 766) + (m >= 1790)


def pack_codes(codes):
    """[(code, width)] -> bytes, MSB first, the last byte padded with zeros."""
    acc = n = 0
    for c, wd in codes:
        acc = (acc << wd) | c
        n += wd
    pad = -n % 8
    return (acc << pad).to_bytes((n + pad) // 8, "big")


def lzw_codes(data, clear_at=(), eoi=True, limit=3837):
    """The LZW codes of `data` as [(code, width)]: a Clear first, another wherever the number of codes written so far is in `clear_at` and once
    `limit` codes follow the last Clear (the table then holds 257 + limit - 1 <= 4093 entries)."""
    codes = []
    m = 0

    def emit(c):
        nonlocal m
        codes.append((c, lzw_width(m)))
        m = 0 if c == 256 else m + 1

    emit(256)
    table = {}
    w = b""
    for byte in bytes(data):
        while not w and len(codes) in clear_at:
            emit(256)
        wc = w + bytes([byte])
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        emit(w[0] if len(w) == 1 else table[w])
        if len(codes) in clear_at or m >= limit:
            emit(256)
            table = {}
        else:
            table[wc] = 257 + m                                  # the entry the decoder makes when it reads the NEXT code
        w = bytes([byte])
    if w:
        emit(w[0] if len(w) == 1 else table[w])
    if eoi:
        emit(257)
    return codes


def lzw_encode(data, clear_at=(), eoi=True, tail=b"", limit=3837):
    return pack_codes(lzw_codes(data, clear_at, eoi, limit)) + tail


def packbits_encode(data):
    """Runs of 3 to 128 equal bytes as run packets, everything else as literals of up to 128 bytes (runs cross row ends freely)."""
    data = bytes(data)
    out = bytearray()
    i, n = 0, len(data)
    lit = bytearray()

    def flush():
        for k in range(0, len(lit), 128):
            part = lit[k:k + 128]
            out.append(len(part) - 1)
            out.extend(part)
        lit.clear()

    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            flush()
            out.append((1 - (j - i)) & 255)
            out.append(data[i])
        else:
            lit.extend(data[i:j])
        i = j
    flush()
    return bytes(out)


def pack(samples, bits):
    """Samples [h, n] (values below 1 << bits) -> rows uint8 [h, ceil(n * bits / 8)], MSB first, padded with zero bits."""
    samples = np.asarray(samples)
    if bits == 8:
        return samples.astype(np.uint8)
    h, n = samples.shape
    per = 8 // bits
    padded = np.zeros((h, -(-n // per) * per), np.int64)
    padded[:, :n] = samples
    shifts = np.arange(per - 1, -1, -1) * bits
    return (padded.reshape(h, -1, per) << shifts).sum(-1).astype(np.uint8)


def difference(rows, w, spp):
    """Predictor 2 applied: every sample minus the sample of the same channel to its left, mod 256."""
    s = rows.reshape(rows.shape[0], w, spp).astype(np.int64)
    s[:, 1:] -= s[:, :-1].copy()
    return (s & 255).astype(np.uint8).reshape(rows.shape)


def assemble(rows, w, bits, spp, photometric, compression=NONE, predictor=1, rows_per_strip=None, byte_order="<", colormap=None, strip_type=LONG,
             size_type=SHORT, level=6, lzw=None, streams=None, extra=None, magic=42):
    """rows: uint8 [h, row_bytes], the packed samples (before the predictor).  rows_per_strip: the tag's value (None: the height; a value above
    the height is written as it is).  strip_type / size_type: the field type of StripOffsets, StripByteCounts and RowsPerStrip / of ImageWidth
    and ImageLength.  lzw: keyword arguments of lzw_encode, or a function of the strip number that returns them.  streams: {strip number: ready-made strip bytes}.
    extra: {tag: (type, [values])} added or replacing, {tag: None} removes.  -> the file's bytes: header | strips | long values | IFD."""
    rows = np.ascontiguousarray(rows, np.uint8)
    h = rows.shape[0]
    tag_rps = h if rows_per_strip is None else rows_per_strip
    rps = min(tag_rps, h)
    body = difference(rows, w, spp) if predictor == 2 else rows
    bo = byte_order
    data = bytearray((b"II" if bo == "<" else b"MM") + struct.pack(bo + "HI", magic, 0))
    offsets, counts = [], []
    for j in range(-(-h // rps)):
        raw = body[j * rps:(j + 1) * rps].tobytes()
        if streams and j in streams:
            z = streams[j]
        elif compression == LZW:
            kw = lzw(j) if callable(lzw) else (lzw or {})
            z = lzw_encode(raw, **kw)
        elif compression in (ADOBE_DEFLATE, DEFLATE):
            z = zlib.compress(raw, level)
        elif compression == PACKBITS:
            z = packbits_encode(raw)
        else:
            z = raw
        offsets.append(len(data))
        counts.append(len(z))
        data += z
        if len(data) & 1:
            data += b"\0"
    tags = {256: (size_type, [w]), 257: (size_type, [h]), 258: (SHORT, [bits] * spp), 259: (SHORT, [compression]), 262: (SHORT, [photometric]),
            273: (strip_type, offsets), 277: (SHORT, [spp]), 278: (strip_type, [tag_rps]), 279: (strip_type, counts)}
    if predictor != 1:
        tags[317] = (SHORT, [predictor])
    if colormap is not None:
        tags[320] = (SHORT, [int(v) for v in colormap])
    for tag, v in (extra or {}).items():
        if v is None:
            tags.pop(tag, None)
        else:
            tags[tag] = v
    entries = b""
    for tag in sorted(tags):
        typ, vals = tags[tag]
        packed = struct.pack(bo + "%d%s" % (len(vals), TYPE_CODE[typ]), *vals)
        if len(packed) <= 4:
            field = packed + bytes(4 - len(packed))              # inline, left-justified
        else:
            field = struct.pack(bo + "I", len(data))
            data += packed
            if len(data) & 1:
                data += b"\0"
        entries += struct.pack(bo + "HHI", tag, typ, len(vals)) + field
    data[4:8] = struct.pack(bo + "I", len(data))
    data += struct.pack(bo + "H", len(tags)) + entries + struct.pack(bo + "I", 0)
    return bytes(data)
