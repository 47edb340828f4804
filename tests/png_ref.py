"""The rule book of the PNG decoder (csrc/png_decode.hip, maf-yolo_amd/png.py) in plain Python / NumPy: chunk walk, inflate, unfilter, conversion.

Every rule, with where it comes from:
* chunks (PNG 1.2, 5.3): length, type, data, CRC-32; the zlib stream is the concatenation of the IDAT payloads (walk() below does its own walk,
  independent of png.parse); the 2-byte zlib header is skipped, the Adler-32 is not read;
* inflate (RFC 1951) with the SAME bounded reader and the SAME status bits as png_inflate_kernel: bits leave the reader least significant first;
  past the end of the stream the reader feeds zeros, and once a bit from there has been CONSUMED the stream ends with INPUT_EXHAUSTED; a
  Huffman code is canonical (3.2.2), a symbol is found by a 9-bit first-level lookup or, for longer codes, a walk over the lengths 10 .. 15
  (counters["long_code"] counts those); a set of code lengths is refused when over-subscribed, or incomplete unless its longest code has 1 bit and
  it is not the code-length code (zlib inftrees.c); more than 286 literal/length or 30 distance codes, a repeat with nothing before it or past the
  end, and a missing end-of-block code are refused too (BAD_CODE_LENGTHS); length symbols 286 / 287 and distance symbols 30 / 31 count as NO_CODE;
  a distance beyond the bytes produced so far is DISTANCE_TOO_FAR; output stops at inflated_size (TOO_MANY_BYTES), a stream that ends before
  it gives TOO_FEW_BYTES; whatever happens the output has exactly inflated_size bytes, zeros behind the last one produced;
* unfilter (PNG 1.2, 6): types 0 .. 4 over bytes at distance bpp = max(1, channels * depth / 8), the row above the first is zeros, Paeth ties go
  to a, then b; a type above 4 sets BAD_FILTER and the row is taken as type 0;
* conversion (what cv2.imread asks libpng for): png_set_strip_16 = the high byte, png_set_expand_gray_1_2_4_to_8 = x 255 / 85 / 17,
  png_set_palette_to_rgb (an index past PLTE: BAD_PALETTE_INDEX, the pixel black), png_set_strip_alpha, gray replicated, BGR.
Stage taps: inflate() -> the filtered scanlines, unfilter() -> the rows, decode_stages() -> all of them.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
(ST_INPUT_EXHAUSTED, ST_BAD_BLOCK_TYPE, ST_BAD_STORED_LEN, ST_BAD_CODE_LENGTHS, ST_NO_CODE, ST_DISTANCE_TOO_FAR, ST_TOO_MANY_BYTES, ST_TOO_FEW_BYTES,
 ST_BAD_FILTER, ST_BAD_PALETTE_INDEX) = (1 << i for i in range(10))
LOOK_BITS = 9
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(typ, body):
    """One chunk with its CRC-32 (the generator and the tests build files with it)."""
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def walk(d):
    """(ihdr fields, palette or None, the zlib stream) of a file; no checks beyond what it needs (png.parse is the checker)."""
    assert d[:8] == SIGNATURE
    p, ihdr, plte, z = 8, None, None, b""
    while p + 8 <= len(d):
        L, = struct.unpack(">I", d[p:p + 4])
        typ, body = d[p + 4:p + 8], d[p + 8:p + 8 + L]
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"IDAT":
            z += body
        elif typ == b"IEND":
            break
        p += 12 + L
    return ihdr, plte, z


class _Bits:
    """The bounded reader: `pos` counts bytes taken into the window (also the zeros past `end`), n the unread bits."""

    def __init__(self, data, begin, end):
        self.d, self.pos, self.end, self.acc, self.n = data, begin, end, 0, 0

    def fill(self):
        while self.n <= 56:
            b = self.d[self.pos] if self.pos < self.end else 0
            self.pos += 1
            self.acc |= b << self.n
            self.n += 8

    def bits(self, k):
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def exhausted(self):
        return self.pos * 8 - self.n > self.end * 8


class _Table:
    """A canonical code: first / count / offs per length, the symbols sorted by (length, symbol)."""

    def __init__(self, lens, code_length_code):
        cnt = [0] * 16
        for l in lens:
            cnt[l] += 1
        cnt[0] = 0
        self.first, self.count, self.offs = [0] * 16, cnt, [0] * 16
        left, code, off, over, maxlen = 1, 0, 0, False, 0
        for b in range(1, 16):
            code <<= 1
            left = 2 * left - cnt[b]
            if left < 0:
                over, left = True, 0
            self.first[b], self.offs[b] = code, off
            if cnt[b]:
                maxlen = b
            code += cnt[b]
            off += cnt[b]
        self.sorted = [s for l in range(1, 16) for s, sl in enumerate(lens) if sl == l]
        self.ok = not over and (left == 0 or (not code_length_code and maxlen <= 1))

    def symbol(self, br, counters):
        br.fill()
        rev = int(format(br.acc & 0x7FFF, "015b")[::-1], 2)        # the next 15 bits, first stream bit most significant
        for l in range(1, 16):
            d = (rev >> (15 - l)) - self.first[l]
            if 0 <= d < self.count[l]:
                if l > LOOK_BITS:
                    counters["long_code"] += 1
                br.bits(l)
                return self.sorted[self.offs[l] + d]
        return -1


_FIXED = None


def new_counters():
    return dict(stored=0, fixed=0, dynamic=0, max_match=0, overlap=0, max_distance=0, long_code=0, filters=[0] * 5)


def inflate(z, size, counters=None, begin=2):
    """The deflate stream z[begin:] -> (uint8 [size], status).  `counters` (new_counters()) collects what the stream reached."""
    global _FIXED
    c = counters if counters is not None else new_counters()
    if _FIXED is None:
        _FIXED = (_Table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _Table([5] * 32, False))
    out = bytearray()
    br = _Bits(z, begin, len(z))
    st, done = 0, False
    max_blocks = (len(z) - begin) * 8 // 3 + 1
    blk = 0
    while blk < max_blocks and not st and not done:
        blk += 1
        br.fill()
        bfinal, btype = br.bits(1), br.bits(2)
        if br.exhausted():
            st |= ST_INPUT_EXHAUSTED
            break
        if btype == 3:
            st |= ST_BAD_BLOCK_TYPE
            break
        if btype == 0:
            br.bits(br.n & 7)
            br.fill()
            ln = br.bits(16)
            br.fill()
            nln = br.bits(16)
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
                break
            if ln ^ 0xFFFF != nln:
                st |= ST_BAD_STORED_LEN
                break
            br.pos -= br.n >> 3
            br.n = br.acc = 0
            take = min(ln, size - len(out))
            out += bytes(br.d[i] if i < br.end else 0 for i in range(br.pos, br.pos + take))
            if br.pos + ln > br.end:
                st |= ST_INPUT_EXHAUSTED
            if ln > take:
                st |= ST_TOO_MANY_BYTES
            br.pos += ln
            c["stored"] += 1
            done = bool(bfinal)
            continue
        ll, dd = _FIXED
        if btype == 2:
            br.fill()
            hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
                break
            if hlit > 286 or hdist > 30:
                st |= ST_BAD_CODE_LENGTHS
                break
            cl_lens = [0] * 19
            for i in range(hclen):
                br.fill()
                cl_lens[CL_ORDER[i]] = br.bits(3)
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
                break
            cl = _Table(cl_lens, True)
            if not cl.ok:
                st |= ST_BAD_CODE_LENGTHS
                break
            lens, prev, it = [], 0, 0
            nsym = hlit + hdist
            while it < 320 and len(lens) < nsym and not st:
                it += 1
                s = cl.symbol(br, c)
                rep, v = 1, s
                if s < 0:
                    st |= ST_NO_CODE
                    break
                if s == 16:
                    if not lens:
                        st |= ST_BAD_CODE_LENGTHS
                        break
                    rep, v = 3 + br.bits(2), prev
                elif s == 17:
                    rep, v = 3 + br.bits(3), 0
                elif s == 18:
                    rep, v = 11 + br.bits(7), 0
                if len(lens) + rep > nsym:
                    st |= ST_BAD_CODE_LENGTHS
                    break
                lens += [v] * rep
                prev = v
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
            if st:
                break
            if lens[256] == 0:
                st |= ST_BAD_CODE_LENGTHS
                break
            ll, dd = _Table(lens[:hlit], False), _Table(lens[hlit:], False)
            if not ll.ok or not dd.ok:
                st |= ST_BAD_CODE_LENGTHS
                break
        c["dynamic" if btype == 2 else "fixed"] += 1
        eob = False
        for _ in range(size + 1):
            s = ll.symbol(br, c)
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
                break
            if s < 0:
                st |= ST_NO_CODE
                break
            if s < 256:
                if len(out) >= size:
                    st |= ST_TOO_MANY_BYTES
                    break
                out.append(s)
                continue
            if s == 256:
                eob = True
                break
            if s > 285:
                st |= ST_NO_CODE
                break
            s -= 257
            L = LEN_BASE[s] + br.bits(LEN_EXTRA[s])
            ds = dd.symbol(br, c)
            if ds < 0 or ds > 29:
                st |= ST_INPUT_EXHAUSTED if br.exhausted() else ST_NO_CODE
                break
            D = DIST_BASE[ds] + br.bits(DIST_EXTRA[ds])
            if br.exhausted():
                st |= ST_INPUT_EXHAUSTED
                break
            if D > len(out):
                st |= ST_DISTANCE_TOO_FAR
                break
            take = min(L, size - len(out))
            p = len(out)
            for i in range(take):
                out.append(out[p - D + i % D])
            c["max_match"] = max(c["max_match"], L)
            c["max_distance"] = max(c["max_distance"], D)
            c["overlap"] += D < L
            if L > take:
                st |= ST_TOO_MANY_BYTES
                break
        if not eob and not st:
            st |= ST_TOO_MANY_BYTES
        if bfinal:
            done = True
    if not done and not st:
        st |= ST_INPUT_EXHAUSTED
    if len(out) < size:
        if not st:
            st |= ST_TOO_FEW_BYTES
        out += bytes(size - len(out))
    return np.frombuffer(bytes(out), np.uint8), st


def unfilter(inflated, h, rowbytes, bpp, counters=None):
    """The filtered scanlines uint8 [h * (1 + rowbytes)] -> (rows uint8 [h, rowbytes], status)."""
    src = inflated.reshape(h, 1 + rowbytes)
    rows = np.zeros((h, rowbytes), np.uint8)
    st = 0
    up = [0] * rowbytes
    for y in range(h):
        ft = int(src[y, 0])
        if ft > 4:
            st |= ST_BAD_FILTER
            ft = 0
        elif counters is not None:
            counters["filters"][ft] += 1
        raw = src[y, 1:].tolist()
        cur = [0] * rowbytes
        for i in range(rowbytes):
            a = cur[i - bpp] if i >= bpp else 0
            b = up[i]
            cc = up[i - bpp] if i >= bpp else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) >> 1
            else:
                pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
            cur[i] = (raw[i] + pred) & 255
        rows[y] = cur
        up = cur
    return rows, st


def convert(rows, w, h, depth, ctype, palette):
    """The rows -> (uint8 [h, w, 3] BGR, status)."""
    st = 0
    ch = CHANNELS[ctype]
    if depth == 16:
        samples = rows.reshape(h, w * ch, 2)[:, :, 0]                            # the high byte
    elif depth == 8:
        samples = rows
    else:
        bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth)   # MSB first
        samples = np.zeros((h, w), np.uint8)
        for k in range(depth):
            samples = (samples << 1) | bits[:, :, k]
    samples = samples.reshape(h, w, ch)
    if ctype == 3:
        idx = samples[:, :, 0].astype(np.int64)
        bad = idx >= len(palette)
        if bad.any():
            st |= ST_BAD_PALETTE_INDEX
        rgb = np.asarray(palette, np.uint8)[np.where(bad, 0, idx)]
        rgb[bad] = 0
        return np.ascontiguousarray(rgb[:, :, ::-1]), st
    if ctype in (0, 4):
        g = samples[:, :, 0]
        if depth < 8:
            g = g * (255 // ((1 << depth) - 1))
        return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8)), st
    return np.ascontiguousarray(samples[:, :, 2::-1]), st


def decode_stages(d, counters=None):
    """A file -> (bgr, inflated, rows, status)."""
    (w, h, depth, ctype, _, _, _), plte, z = walk(d)
    ch = CHANNELS[ctype]
    rowbytes = (w * ch * depth + 7) // 8
    inflated, st = inflate(z, h * (1 + rowbytes), counters)
    rows, st2 = unfilter(inflated, h, rowbytes, max(1, ch * depth // 8), counters)
    bgr, st3 = convert(rows, w, h, depth, ctype, plte)
    return bgr, inflated, rows, st | st2 | st3


def decode(d):
    bgr, _, _, st = decode_stages(d)
    assert st == 0, "status 0x%x" % st
    return bgr


# ---------------------------------------------------------------- the writer side (fixtures and tests build their files with it)

def filter_rows(rows, filters, bpp):
    """rows uint8 [h, rowbytes] + a filter type per row -> the filtered scanlines uint8 [h * (1 + rowbytes)] (PNG 1.2, 6, the encoder's direction)."""
    h, rb = rows.shape
    out = np.zeros((h, 1 + rb), np.uint8)
    r = rows.astype(np.int32)
    zero = np.zeros(rb, np.int32)
    for y in range(h):
        ft = filters[y % len(filters)]
        cur, up = r[y], (r[y - 1] if y else zero)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])[:rb] if rb > bpp else np.zeros(rb, np.int32)
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        elif ft == 4:
            pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        else:                                                  # not a PNG filter: the malformed fixtures store the row as it is
            pred = zero
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.reshape(-1)


def ihdr(w, h, depth, ctype, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, compression, filt, interlace))


def assemble(w, h, depth, ctype, zstream, palette=None, before_idat=b"", split=None, **kw):
    """signature | IHDR | [PLTE] | before_idat | IDAT ... | IEND; split = n cuts the zlib stream into IDAT chunks of n bytes."""
    n = len(zstream) if not split else split
    idat = b"".join(chunk(b"IDAT", zstream[i:i + n]) for i in range(0, len(zstream), n)) if zstream else chunk(b"IDAT", b"")
    plte = chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()) if palette is not None else b""
    return SIGNATURE + ihdr(w, h, depth, ctype, **kw) + plte + before_idat + idat + chunk(b"IEND", b"")


def encode(rows, w, depth, ctype, filters=(0, 1, 2, 3, 4), level=9, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_at=None, **kw):
    """rows uint8 [h, rowbytes] (the packed samples of the file) -> (the file, its filtered scanlines).  flush_at: a Z_FULL_FLUSH behind that many bytes."""
    ch = CHANNELS[ctype]
    raw = filter_rows(rows, filters, max(1, ch * depth // 8)).tobytes()
    co = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    if flush_at:
        z = co.compress(raw[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[flush_at:]) + co.flush()
    else:
        z = co.compress(raw) + co.flush()
    return assemble(w, rows.shape[0], depth, ctype, z, **kw), np.frombuffer(raw, np.uint8)
