"""The BMP rule book in numpy, a hand assembler that writes a BMP file from pixels or RLE records, and the `rewrite` transcoder.  No GPU, no
Pillow.

What maf-yolo_amd/bmp.py and csrc/bmp_decode.hip compute, restated serially (checked against Pillow by tools/make_golden_bmp.py and
tests/test_bmp_host.py):
  * read_header(d)     the file header and the DIB header (12, 40, 52, 56, 64, 108 or 124 bytes) -> a dict;
  * records(stream)    the RLE records one after the other: ("run", n, v), ("eol",), ("eob",), ("delta", dx, dy), ("abs", n, payload bytes);
                       every record has an even length (an absolute payload is padded to even);
  * rle_decode         a position (x, y) in file rows: a run writes from x and moves right (RLE4: the nibbles of v, or of the payload, in turn,
                       an odd absolute count n reads ceil(n / 2) bytes and yields n pixels); eol: x = 0, y + 1 (a full row stays on its row
                       until it comes, on an empty row it skips the row); delta: x + dx, y + dy; eob ends the image; pixels nothing writes are
                       index 0; the walk stops once the position is at or past the last pixel (y >= h, or the last row full).  A record whose
                       bytes lie past the data is ST_INPUT_EXHAUSTED, a run past its row's end is clamped there and ST_RUN_PAST_ROW, a delta to
                       x > w or y >= h ST_DELTA_PAST_IMAGE; each ends the walk;
  * decode_stages(d)   -> (BGR uint8 [h, w, 3], the index plane uint8 [h, w] in file row order (None for uncompressed data), the status word):
                       rows padded to 4 bytes, bottom-up unless the height is negative, 1 / 4 bit MSB first, palette entries B, G, R, x (an index
                       at or above `colors` is black), 24 bit B, G, R, 32 bit B, G, R and a 4th byte that is dropped.
The assembler: pack_rows packs pixels into padded rows in file order; assemble writes any header kind around ready-made pixel data; rle_stream
writes records; rle_records is a plain encoder (runs of three and more, absolute runs for the rest, an end of line per row).
rewrite(file): the same picture without the three constructs Pillow 12.2 reads differently from the rule: an odd RLE4 absolute run becomes an
even one (or a 2-pixel encoded run) plus a 1-pixel encoded run, an end of line on an empty row becomes delta (0, 1), an early end of bitmap
becomes deltas and an end of line that reach the last pixel.
"""
import struct

import numpy as np

ST_INPUT_EXHAUSTED, ST_RUN_PAST_ROW, ST_DELTA_PAST_IMAGE = 1, 2, 4
RGB, RLE8, RLE4, BITFIELDS = 0, 1, 2, 3
HEADER_SIZES = (12, 40, 52, 56, 64, 108, 124)


# ---------------------------------------------------------------- reading

def read_header(d):
    """-> dict(offset, header, width, height (positive), top_down, planes, bits, compression, colors (as stored), entry (palette entry bytes))."""
    assert d[:2] == b"BM"
    off, hs = struct.unpack("<I", d[10:14])[0], struct.unpack("<I", d[14:18])[0]
    if hs == 12:
        w, h, planes, bits = struct.unpack("<HHHH", d[18:26])
        comp, colors, entry = RGB, 0, 3
    else:
        w, h, planes, bits, comp = struct.unpack("<iiHHI", d[18:34])
        colors, = struct.unpack("<I", d[46:50])
        entry = 4
    return dict(offset=off, header=hs, width=w, height=abs(h), top_down=h < 0, planes=planes, bits=bits, compression=comp, colors=colors, entry=entry)


def records(stream, rle4):
    """The records of an RLE stream, serially -> [(offset, record)]; a record whose bytes lie past the data ends the list with (offset, None)."""
    out, o, n = [], 0, len(stream)
    while True:
        if o + 2 > n:
            out.append((o, None))
            return out
        b0, b1 = stream[o], stream[o + 1]
        if b0:
            out.append((o, ("run", b0, b1)))
            o += 2
        elif b1 == 0:
            out.append((o, ("eol",)))
            o += 2
        elif b1 == 1:
            out.append((o, ("eob",)))
            return out
        elif b1 == 2:
            if o + 4 > n:
                out.append((o, None))
                return out
            out.append((o, ("delta", stream[o + 2], stream[o + 3])))
            o += 4
        else:
            nb = (b1 + 1) // 2 if rle4 else b1
            if o + 2 + nb > n:
                out.append((o, None))
                return out
            out.append((o, ("abs", b1, bytes(stream[o + 2:o + 2 + nb]))))
            o += 2 + (nb + 1) // 2 * 2


def _pixels(rec, rle4):
    """The index values a run record yields."""
    if rec[0] == "run":
        n, v = rec[1], rec[2]
        return [((v >> 4) if j % 2 == 0 else v & 15) for j in range(n)] if rle4 else [v] * n
    n, pay = rec[1], rec[2]
    return [((pay[j // 2] >> 4) if j % 2 == 0 else pay[j // 2] & 15) for j in range(n)] if rle4 else list(pay[:n])


def _complete(x, y, w, h):
    return y >= h or (y == h - 1 and x >= w)


def walk(stream, w, h, rle4):
    """The rule: yields (record, x, y in front of it) for every record that is carried out, then returns the status through StopIteration."""
    x = y = 0
    for _, rec in records(stream, rle4):
        if _complete(x, y, w, h):
            return 0
        if rec is None:
            return ST_INPUT_EXHAUSTED
        if rec[0] == "eob":
            yield rec, x, y
            return 0
        if rec[0] == "delta" and (x + rec[1] > w or y + rec[2] >= h):
            return ST_DELTA_PAST_IMAGE
        yield rec, x, y
        if rec[0] == "eol":
            x, y = 0, y + 1
        elif rec[0] == "delta":
            x, y = x + rec[1], y + rec[2]
        else:
            if x + rec[1] > w:
                return ST_RUN_PAST_ROW
            x += rec[1]
    return 0


def rle_decode(stream, w, h, rle4):
    """-> (the index plane uint8 [h, w] in file row order, the status word)."""
    plane = np.zeros((h, w), np.uint8)
    g = walk(stream, w, h, rle4)
    while True:
        try:
            rec, x, y = next(g)
        except StopIteration as e:
            return plane, e.value
        if rec[0] in ("run", "abs"):
            px = _pixels(rec, rle4)[:max(0, w - x)]
            plane[y, x:x + len(px)] = px


def decode_stages(d):
    """-> (BGR uint8 [h, w, 3], the index plane or None, the status word) of a file of the supported set."""
    d = bytes(d)
    hd = read_header(d)
    w, h, bits, comp, off = hd["width"], hd["height"], hd["bits"], hd["compression"], hd["offset"]
    pal = None
    if bits <= 8:
        colors = hd["colors"] or 1 << bits
        at = 14 + hd["header"]
        e = np.frombuffer(d, np.uint8, hd["entry"] * colors, at).reshape(colors, hd["entry"])[:, :3]
        pal = np.zeros((256, 3), np.uint8)
        pal[:colors] = e
    plane, st = None, 0
    if comp in (RLE8, RLE4):
        plane, st = rle_decode(d[off:], w, h, comp == RLE4)
        idx = plane
    else:
        stride = (w * bits + 31) // 32 * 4
        rows = np.frombuffer(d, np.uint8, h * stride, off).reshape(h, stride)
        if bits == 8:
            idx = rows[:, :w]
        elif bits == 4:
            idx = np.stack([rows >> 4, rows & 15], -1).reshape(h, -1)[:, :w]
        elif bits == 1:
            idx = np.unpackbits(rows, axis=1)[:, :w]
        else:
            idx = None
            bgr = rows[:, :w * bits // 8].reshape(h, w, bits // 8)[:, :, :3]
    if idx is not None:
        bgr = pal[idx]
    if not hd["top_down"]:
        bgr = bgr[::-1]
    return np.ascontiguousarray(bgr), plane, st


def decode(d):
    return decode_stages(d)[0]


# ---------------------------------------------------------------- writing

def pack_rows(px, bits, top_down=False):
    """Pixels in picture order (indices [h, w] at 1 / 4 / 8 bits, bytes [h, w, 3] B, G, R at 24, [h, w, 4] at 32) -> the pixel data: rows padded
    to 4 bytes, bottom-up unless top_down."""
    px = np.asarray(px)
    h, w = px.shape[:2]
    if bits == 8:
        rows = px.astype(np.uint8)
    elif bits == 4:
        p = np.zeros((h, (w + 1) // 2 * 2), np.uint8)
        p[:, :w] = px
        rows = (p[:, 0::2] << 4 | p[:, 1::2]).astype(np.uint8)
    elif bits == 1:
        rows = np.packbits(px.astype(np.uint8), axis=1)
    else:
        rows = px.astype(np.uint8).reshape(h, -1)
    stride = (w * bits + 31) // 32 * 4
    out = np.zeros((h, stride), np.uint8)
    out[:, :rows.shape[1]] = rows
    return (out if top_down else out[::-1]).tobytes()


def assemble(w, h, bits, data, header=40, compression=RGB, top_down=False, palette=None, colors=None, gap=0, masks=None, alpha=None, planes=1, offset=None):
    """A BMP file around ready-made pixel data.  palette: [k, 3] B, G, R entries (written with 3 bytes each behind a 12-byte header, else 4);
    colors: the header's biClrUsed (default: 0 where the palette is full, else its length); gap: bytes between the palette and the pixel data;
    masks: the three BITFIELDS masks (behind a 40-byte header, inside a longer one), alpha: the 4th (headers of 56 bytes and more);
    offset: overrides bfOffBits."""
    if header == 12:
        dib = struct.pack("<IHHHH", 12, w, h, planes, bits)
    else:
        if colors is None:
            colors = 0 if palette is None or len(palette) == 1 << bits else len(palette)
        dib = struct.pack("<IiiHHIIiiII", header, w, -h if top_down else h, planes, bits, compression, len(data), 2835, 2835, colors, 0)
        rest = bytearray(header - 40)
        if masks is not None and header >= 52:
            rest[0:12] = struct.pack("<III", *masks)
            if header >= 56:
                rest[12:16] = struct.pack("<I", alpha or 0)
        dib += bytes(rest)
        if masks is not None and header == 40:
            dib += struct.pack("<III", *masks)
    pal = b""
    if palette is not None:
        e = np.zeros((len(palette), 3 if header == 12 else 4), np.uint8)
        e[:, :3] = palette
        pal = e.tobytes()
    off = 14 + len(dib) + len(pal) + gap if offset is None else offset
    body = dib + pal + bytes([0xEE]) * gap + bytes(data)
    return b"BM" + struct.pack("<IHHI", 14 + len(body), 0, 0, off) + body


def rle_stream(recs, rle4):
    """Records -> bytes.  ("run", n, v), ("eol",), ("eob",), ("delta", dx, dy), ("abs", [index values]) (3 to 255 of them), ("raw", bytes)."""
    out = bytearray()
    for r in recs:
        if r[0] == "run":
            out += bytes([r[1], r[2]])
        elif r[0] == "eol":
            out += b"\0\0"
        elif r[0] == "eob":
            out += b"\0\1"
        elif r[0] == "delta":
            out += bytes([0, 2, r[1], r[2]])
        elif r[0] == "raw":
            out += r[1]
        else:
            px = [int(v) for v in r[1]]
            assert 3 <= len(px) <= 255
            if rle4:
                px2 = px + [0] * (len(px) % 2)
                pay = bytes(px2[i] << 4 | px2[i + 1] for i in range(0, len(px2), 2))
            else:
                pay = bytes(px)
            out += bytes([0, len(px)]) + pay + bytes(len(pay) % 2)
    return bytes(out)


def rle_records(plane, rle4, abs_max=255, eol_last=False):
    """A plain encoder: an index plane [h, w] in file row order -> records (runs of three and more, absolute runs of up to abs_max for the rest,
    an end of line behind every row but (unless eol_last) the last, an end of bitmap)."""
    plane = np.asarray(plane)
    h, w = plane.shape
    recs = []
    for y in range(h):
        row = [int(v) for v in plane[y]]
        x, lit = 0, []

        def flush():
            while lit:
                take = lit[:abs_max]
                if rle4 and len(take) >= 3 and len(take) % 2:   # an even count: Pillow reads an odd RLE4 absolute run differently
                    take = take[:-1]
                del lit[:len(take)]
                if len(take) >= 3:
                    recs.append(("abs", take))
                else:
                    recs.extend(("run", 1, v << 4 if rle4 else v) for v in take)
        while x < w:
            n = 1                                              # an RLE4 run alternates two nibbles, so its second pixel is free
            while x + n < w and n < 255 and ((rle4 and n < 2) or row[x + n] == row[x + (n % 2 if rle4 else 0)]):
                n += 1
            if n >= 3:
                flush()
                recs.append(("run", n, (row[x] << 4 | row[x + 1]) if rle4 else row[x]))
                x += n
            else:
                lit.append(row[x])
                x += 1
        flush()
        if y < h - 1 or eol_last:
            recs.append(("eol",))
    recs.append(("eob",))
    return recs


def rle_file(w, h, recs, rle4, palette, **kw):
    """A BI_RLE8 / BI_RLE4 file from records."""
    return assemble(w, h, 4 if rle4 else 8, rle_stream(recs, rle4), compression=RLE4 if rle4 else RLE8, palette=palette, **kw)


# ---------------------------------------------------------------- the rewrite

def _to_the_end(x, y, w, h):
    """Records that move from (x, y) to the last pixel's end without writing: deltas up to the last row, then an end of line (deltas to the
    right where the row is empty: an end of line there is what Pillow ignores)."""
    out = []
    while y < h - 1:
        up = min(255, h - 1 - y)
        out.append(("delta", 0, up))
        y += up
    if x > 0:
        out.append(("eol",))
    else:
        while x < w:
            right = min(255, w - x)
            out.append(("delta", right, 0))
            x += right
    return out


def departs(d):
    """The constructs of a file on which Pillow 12.2 departs from the rule -> a sorted list out of "odd_rle4_absolute", "empty_row_eol",
    "early_eob" (empty for uncompressed files)."""
    d = bytes(d)
    hd = read_header(d)
    if hd["compression"] not in (RLE8, RLE4):
        return []
    w, h, rle4 = hd["width"], hd["height"], hd["compression"] == RLE4
    found = set()
    for rec, x, y in walk(d[hd["offset"]:], w, h, rle4):
        if rec[0] == "abs" and rle4 and rec[1] % 2:
            found.add("odd_rle4_absolute")
        elif rec[0] == "eol" and x == 0:
            found.add("empty_row_eol")
        elif rec[0] == "eob" and not _complete(x, y, w, h):
            found.add("early_eob")
    return sorted(found)


def rewrite(d):
    """An RLE file whose stream is well-formed -> a file with the same rule-book pixels that Pillow 12.2 reads by the rule (see the module text)."""
    d = bytes(d)
    hd = read_header(d)
    w, h, rle4 = hd["width"], hd["height"], hd["compression"] == RLE4
    assert hd["compression"] in (RLE8, RLE4)
    out = []
    g = walk(d[hd["offset"]:], w, h, rle4)
    ended = False
    x = y = 0
    while True:
        try:
            rec, x, y = next(g)
        except StopIteration as e:
            assert e.value == 0, "rewrite takes well-formed streams only"
            break
        if rec[0] == "abs":
            px = _pixels(rec, rle4)
            if rle4 and len(px) % 2:
                even = px[:-1]
                out.append(("run", 2, even[0] << 4 | even[1]) if len(even) == 2 else ("abs", even))
                out.append(("run", 1, px[-1] << 4))
            else:
                out.append(("abs", px))
            x += len(px)
        elif rec[0] == "eol" and x == 0:
            out += [("delta", 0, 1)] if y < h - 1 else _to_the_end(x, y, w, h)
            y += 1
        elif rec[0] == "eob":
            out += _to_the_end(x, y, w, h)
            ended = True
        else:
            out.append(rec)
            if rec[0] == "run":
                x += rec[1]
            elif rec[0] == "delta":
                x, y = x + rec[1], y + rec[2]
            else:
                x, y = 0, y + 1
    if not ended and not _complete(x, y, w, h):                 # cannot happen on a well-formed stream: status 0 means eob or complete
        out += _to_the_end(x, y, w, h)
    out.append(("eob",))
    return d[:hd["offset"]] + rle_stream(out, rle4)
