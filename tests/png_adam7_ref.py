"""The rule book of Adam7 PNG decoding (png.decode(..., interlaced=True), csrc/png_decode.hip) in plain Python / NumPy, on top of tests/png_ref.py.

Every rule, with where it comes from (PNG 1.2, 8.2 and 6.1):
* pass p = 1 .. 7 holds the pixels (x0 + i * dx, y0 + j * dy) of the image, (x0, y0, dx, dy) from PASSES below, as a sub-image of pw x ph pixels,
  pw = ceil((w - x0) / dx), ph = ceil((h - y0) / dy), whose rows are packed like those of a plain image: prb = ceil(pw * channels * depth / 8)
  bytes, sub-byte pixels MSB first, the last byte of a row padded;
* every pass is filtered on its own (its first row has zeros above it, the filters' byte distance bpp is the image's); the filtered passes
  follow each other in ONE zlib stream; a pass with pw == 0 or ph == 0 is absent, filter bytes included;
* so the inflated size is the sum of ph * (1 + prb) over the non-empty passes, and the status bits of png_ref.inflate (TOO_FEW / TOO_MANY ...)
  are relative to that sum; BAD_FILTER is found in any pass (the row is taken as type 0);
* the unfiltered sub-images lie back to back (the `rows` tap of the device); pixel (x, y) of the image is pixel ((x - x0) / dx, (y - y0) / dy)
  of the one pass whose lattice holds it; the conversion of png_ref.convert follows.
The writer side (split, encode) builds the files of tools/make_golden_png_adam7.py: Pillow reads Adam7 but cannot write it.
"""
import zlib

import numpy as np

import png_ref as R

PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def geometry(w, h, bits):
    """[(x0, y0, dx, dy, pw, ph, prb)] of the seven passes (pw or ph may be 0)."""
    out = []
    for x0, y0, dx, dy in PASSES:
        pw, ph = len(range(x0, w, dx)), len(range(y0, h, dy))
        out.append((x0, y0, dx, dy, pw, ph, (pw * bits + 7) // 8))
    return out


def sizes(w, h, bits):
    """(inflated size, bytes of the unfiltered sub-images back to back)."""
    live = [(ph, prb) for _, _, _, _, pw, ph, prb in geometry(w, h, bits) if pw and ph]
    return sum(ph * (1 + prb) for ph, prb in live), sum(ph * prb for ph, prb in live)


def unpack_pixels(rows, w, depth, ch):
    """Packed rows uint8 [h, rowbytes] -> pixels uint8 [h, w, k]: the k = channels * depth / 8 bytes of a pixel, or below 8 bits its one value."""
    h = rows.shape[0]
    if depth >= 8:
        k = ch * depth // 8
        return rows[:, :w * k].reshape(h, w, k)
    bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth)
    v = np.zeros((h, w), np.uint8)
    for b in range(depth):
        v = (v << 1) | bits[:, :, b]
    return v[:, :, None]


def pack_pixels(px, depth):
    """The inverse of unpack_pixels: pixels [h, w, k] -> packed rows uint8 [h, rowbytes] (MSB first, the last byte padded with zeros)."""
    h, w, k = px.shape
    if depth >= 8:
        return np.ascontiguousarray(px).reshape(h, w * k)
    bits = ((px.reshape(h, w, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, w * depth)
    return np.packbits(bits, axis=1) if w else np.zeros((h, 0), np.uint8)


def unfilter(inflated, w, h, depth, ctype, counters=None):
    """The inflated stream of an Adam7 image -> ([the unfiltered sub-image uint8 [ph, prb] of every pass, None where absent], status)."""
    ch = R.CHANNELS[ctype]
    bpp = max(1, ch * depth // 8)
    subs, st, at = [], 0, 0
    for _, _, _, _, pw, ph, prb in geometry(w, h, ch * depth):
        if not pw or not ph:
            subs.append(None)
            continue
        n = ph * (1 + prb)
        sub, s = R.unfilter(inflated[at:at + n], ph, prb, bpp, counters)
        subs.append(sub)
        st |= s
        at += n
    assert at == inflated.size
    return subs, st


def deinterlace(subs, w, h, depth, ctype):
    """The sub-images -> the packed rows uint8 [h, rowbytes] a plain file of the same pixels would hold."""
    ch = R.CHANNELS[ctype]
    px = np.zeros((h, w, max(1, ch * depth // 8)), np.uint8)
    for (x0, y0, dx, dy, pw, ph, prb), sub in zip(geometry(w, h, ch * depth), subs):
        if sub is not None:
            px[y0::dy, x0::dx] = unpack_pixels(sub, pw, depth, ch)
    return pack_pixels(px, depth)


def decode_stages(d, counters=None):
    """An Adam7 file -> (bgr, inflated, the sub-images back to back uint8 [n], status)."""
    (w, h, depth, ctype, _, _, lace), plte, z = R.walk(d)
    assert lace == 1
    ch = R.CHANNELS[ctype]
    inflated, st = R.inflate(z, sizes(w, h, ch * depth)[0], counters)
    subs, st2 = unfilter(inflated, w, h, depth, ctype, counters)
    bgr, st3 = R.convert(deinterlace(subs, w, h, depth, ctype), w, h, depth, ctype, plte)
    flat = np.concatenate([s.reshape(-1) for s in subs if s is not None])
    return bgr, inflated, flat, st | st2 | st3


def decode(d):
    bgr, _, _, st = decode_stages(d)
    assert st == 0, "status 0x%x" % st
    return bgr


# ---------------------------------------------------------------- the writer side

def split(rows, w, depth, ctype):
    """Packed rows uint8 [h, rowbytes] of an image -> the packed sub-image uint8 [ph, prb] of every pass (None where absent)."""
    ch = R.CHANNELS[ctype]
    h = rows.shape[0]
    px = unpack_pixels(rows, w, depth, ch)
    return [pack_pixels(px[y0::dy, x0::dx], depth) if pw and ph else None for x0, y0, dx, dy, pw, ph, _ in geometry(w, h, ch * depth)]


def filtered(rows, w, depth, ctype, cycle=5):
    """The filtered scanlines of the Adam7 image: row r of pass p (counted from 0) takes filter type (r + p) % cycle, so that with cycle = 5
    Average and Paeth meet a pass's first row; cycle = 1 is filter 0 throughout."""
    bpp = max(1, R.CHANNELS[ctype] * depth // 8)
    parts = []
    for p, sub in enumerate(split(rows, w, depth, ctype)):
        if sub is not None:
            parts.append(R.filter_rows(sub, [(r + p) % cycle for r in range(sub.shape[0])], bpp))
    return np.concatenate(parts)


def encode(rows, w, depth, ctype, cycle=5, level=9, **kw):
    """Packed rows uint8 [h, rowbytes] -> (the Adam7 file, its filtered scanlines)."""
    raw = filtered(rows, w, depth, ctype, cycle)
    return R.assemble(w, rows.shape[0], depth, ctype, zlib.compress(raw.tobytes(), level), interlace=1, **kw), raw
