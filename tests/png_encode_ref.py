"""The rule book of the PNG encoder (csrc/png_encode.hip, maf-yolo_amd/png_encode.py) in plain Python / NumPy: filter, tokens, blocks, trees,
bits, Adler-32, file.  Its judge is the interpreter's zlib module: zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE) over the filtered
bytes (tests/test_png_encode_host.py); the stream begins 78 01.

Every rule, with where it comes from (zlib 1.2.11):
* filter (PNG 1.2, 6): R, G, B bytes per pixel, ONE filter type for every row of a file, the type byte in front of each row, the row above the
  first is zeros, Paeth ties go to a, then b (png_ref.filter_rows);
* tokens (deflate.c deflate_rle): matches at distance 1 only.  A maximal run of R equal bytes (it starts at byte 0 or at a byte that differs
  from the one before; runs cross rows and include the type bytes) gives one literal, then with r = R - 1: while r >= 3 a match of
  min(258, r) bytes, then r < 3 literals.  A token here is an int: below 256 the literal, 256 + length a match;
* blocks (deflate.h _tr_tally): a block closes after LIT_BUFSIZE - 1 = 16383 symbols, the last block holds the rest; when the symbol count is a
  multiple of 16383 that is an EMPTY last block (deflate_rle ends with FLUSH_BLOCK(s, 1) whatever is pending);
* block type (trees.c _tr_flush_block, level > 0): opt_lenb = (opt_len + 3 + 7) >> 3, static_lenb likewise; opt_lenb = min of the two; stored
  when stored_len + 4 <= opt_lenb, else fixed when static_lenb == opt_lenb, else dynamic.
  zlib writes no stored block once block_start has slid below the window (buf == NULL).  That never binds here: stored wins only when
  lit + 3 * m + 4 <= (9 * lit + 18 * m + 10) / 8 at the least (lit literals and m matches; a literal costs at most 9 static bits, a match at
  distance 1 at most 8 + 5 + 5, and covers at least 3 bytes), so lit >= 6 * m + 22, and with lit + m <= 16383 the static form is at most
  (9 * 14043 + 18 * 2340 + 10) / 8 = 21064 bytes, which bounds stored_len; the window slides when strstart reaches wsize + MAX_DIST = 65274, and
  block_start falls below 0 only if it was below 32768 then, that is when the block already spans more than 32506 bytes.  deflate() asserts
  stored_len < 32768 - 262 on every stored block all the same;
* trees (trees.c): build_tree (heap filled in symbol order, smaller(): the lower frequency, on a tie depth[n] <= depth[m]; fewer than two used
  codes: node = max_code < 2 ? ++max_code : 0 is forced with frequency 1, opt_len-- and static_len -= its static length), gen_bitlen with the
  overflow repair (max 15 bits; 7 for the bit-length tree), gen_codes (bit-reversed: deflate sends Huffman codes most significant bit first
  into a least-significant-first stream), scan_tree / send_tree (138/3 after a zero, 6/3 after an equal length, else 7/4), bl_order, max_blindex
  counted down to 3, opt_len += 3 * (max_blindex + 1) + 14.  Every tally has end-of-block with frequency 1; distance 1 is distance code 0.
  The 7-bit limit of the bit-length tree IS reached by ordinary streams (some hundred literal values with Fibonacci-like frequencies spread the
  code lengths over 1 .. 15 with Fibonacci-like counts): targeted_frames()["bl_limit"] is one, and the host test asserts that it takes the repair;
* tail: the bit buffer is flushed to a byte, then the Adler-32 of the filtered bytes, big-endian;
* file (ours, not libpng's): signature, IHDR (8 bit, colour type 2, 0, 0, 0), ONE IDAT with the whole stream, IEND.
encode() -> the file, and through `taps`: raw (filtered bytes), tokens, blocks (type, first symbol, symbols, bits), bitoff, zstream.
"""
import struct
import zlib

import numpy as np

import png_ref

FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}
LIT_BUFSIZE = 1 << (8 + 6)
BLOCK_SYMBOLS = LIT_BUFSIZE - 1
STORED, FIXED, DYNAMIC = 0, 1, 2
L_CODES, D_CODES, BL_CODES, HEAP_SIZE, END_BLOCK = 286, 30, 19, 573, 256
EXTRA_BL = [0] * 16 + [2, 3, 7]
STATIC_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
STATIC_D = [5] * 30
LEN_CODE = np.zeros(259, np.int64)                         # match length -> index into LEN_BASE (trees.c _length_code)
for _i, _b in enumerate(png_ref.LEN_BASE):
    LEN_CODE[_b:] = _i


def filtered(bgr, filt="sub"):
    """uint8 [h, w, 3] BGR -> the filtered scanlines uint8 [h * (1 + 3 * w)]."""
    h, w = bgr.shape[:2]
    return png_ref.filter_rows(np.ascontiguousarray(bgr[..., ::-1]).reshape(h, 3 * w), (FILTERS[filt],), 3)


def frame_for_stream(stream, w, h):
    """The BGR frame [h, w, 3] whose Sub-filtered bytes are `stream` (uint8 [h * (1 + 3 * w)]; every type byte, stream[y * (1 + 3 * w)], must be 1)."""
    s = np.asarray(stream, np.uint8).reshape(h, 1 + 3 * w)
    assert (s[:, 0] == 1).all(), "a Sub-filtered stream has the type byte 1 at every row start"
    rgb = np.cumsum(s[:, 1:].reshape(h, w, 3).astype(np.int64), axis=1).astype(np.uint8)
    return np.ascontiguousarray(rgb[..., ::-1])


def tokenise(raw):
    """The run rule -> int32 tokens (below 256: literal; 256 + length: match at distance 1)."""
    raw = np.asarray(raw, np.uint8)
    start = np.flatnonzero(np.concatenate([[True], raw[1:] != raw[:-1]]))
    R = np.diff(np.concatenate([start, [raw.size]]))
    q, rem = np.divmod(R - 1, 258)
    ntok = 1 + q + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(R.size), ntok)
    k = np.arange(int(ntok.sum())) - np.repeat(np.cumsum(ntok) - ntok, ntok)
    val = raw[start][run].astype(np.int32)
    return np.where(k == 0, val, np.where(k <= q[run], 256 + 258, np.where(rem[run] >= 3, 256 + rem[run], val))).astype(np.int32)


class _State:
    def __init__(self):
        self.opt_len = self.static_len = 0
        self.overflow = []                                  # per build_tree call: the codes gen_bitlen found beyond max_length


def build_tree(freq, elems, stree, extra, base, max_length, st):
    """trees.c build_tree + gen_bitlen -> (code lengths [elems], max_code).  freq: the elems frequencies (not modified)."""
    freq = list(freq) + [0] * (HEAP_SIZE - elems)
    dad, length, depth = [0] * HEAP_SIZE, [0] * HEAP_SIZE, [0] * HEAP_SIZE
    heap = [0] * (HEAP_SIZE + 1)
    n_heap, heap_max, max_code = 0, HEAP_SIZE, -1

    def smaller(n, m):
        return freq[n] < freq[m] or (freq[n] == freq[m] and depth[n] <= depth[m])

    def down(k):
        v, j = heap[k], k << 1
        while j <= n_heap:
            if j < n_heap and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k, j = j, j << 1
        heap[k] = v

    for n in range(elems):
        if freq[n]:
            n_heap += 1
            heap[n_heap] = max_code = n
    while n_heap < 2:
        if max_code < 2:
            max_code += 1
            node = max_code
        else:
            node = 0
        n_heap += 1
        heap[n_heap] = node
        freq[node] = 1
        st.opt_len -= 1
        if stree:
            st.static_len -= stree[node]
    for n in range(n_heap // 2, 0, -1):
        down(n)
    node = elems
    while True:
        n = heap[1]
        heap[1] = heap[n_heap]
        n_heap -= 1
        down(1)
        m = heap[1]
        heap_max -= 1
        heap[heap_max] = n
        heap_max -= 1
        heap[heap_max] = m
        freq[node] = freq[n] + freq[m]
        depth[node] = max(depth[n], depth[m]) + 1
        dad[n] = dad[m] = node
        heap[1] = node
        node += 1
        down(1)
        if n_heap < 2:
            break
    heap_max -= 1
    heap[heap_max] = heap[1]
    # gen_bitlen
    bl_count = [0] * 16
    length[heap[heap_max]] = 0
    overflow = 0
    for h in range(heap_max + 1, HEAP_SIZE):
        n = heap[h]
        bits = length[dad[n]] + 1
        if bits > max_length:
            bits, overflow = max_length, overflow + 1
        length[n] = bits
        if n > max_code:
            continue
        bl_count[bits] += 1
        xbits = extra[n - base] if n >= base else 0
        st.opt_len += freq[n] * (bits + xbits)
        if stree:
            st.static_len += freq[n] * (stree[n] + xbits)
    st.overflow.append(overflow)
    if overflow:
        while overflow > 0:
            bits = max_length - 1
            while bl_count[bits] == 0:
                bits -= 1
            bl_count[bits] -= 1
            bl_count[bits + 1] += 2
            bl_count[max_length] -= 1
            overflow -= 2
        h = HEAP_SIZE
        for bits in range(max_length, 0, -1):
            n = bl_count[bits]
            while n:
                h -= 1
                m = heap[h]
                if m > max_code:
                    continue
                if length[m] != bits:
                    st.opt_len += (bits - length[m]) * freq[m]
                    length[m] = bits
                n -= 1
    return length[:elems], max_code


def gen_codes(lengths, max_code):
    """trees.c gen_codes: the canonical codes of the lengths, bit-reversed -> list [len(lengths)]."""
    count = [0] * 16
    for n in range(max_code + 1):
        count[lengths[n]] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lengths)
    for n in range(max_code + 1):
        b = lengths[n]
        if b:
            out[n] = int(format(nxt[b], "0%db" % b)[::-1], 2)
            nxt[b] += 1
    return out


def _walk_tree(lengths, max_code, emit):
    """The loop scan_tree and send_tree share: emit(symbol of the bit-length alphabet, repeat count or None)."""
    lens = list(lengths[:max_code + 1]) + [0xFFFF]
    prevlen, nextlen, count = -1, lens[0], 0
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for n in range(max_code + 1):
        curlen, nextlen = nextlen, lens[n + 1]
        count += 1
        if count < max_count and curlen == nextlen:
            continue
        if count < min_count:
            for _ in range(count):
                emit(curlen, None)
        elif curlen != 0:
            if curlen != prevlen:
                emit(curlen, None)
                count -= 1
            emit(16, count)
        elif count <= 10:
            emit(17, count)
        else:
            emit(18, count)
        count, prevlen = 0, curlen
        max_count, min_count = (138, 3) if nextlen == 0 else ((6, 3) if curlen == nextlen else (7, 4))


def block_plan(tokens):
    """Everything _tr_flush_block decides for one block's tokens -> dict(type, bits without the stored padding, the fields that follow the 3
    header bits as (value, nbits) arrays for a fixed or dynamic block, stored_len)."""
    tokens = np.asarray(tokens, np.int64)
    lit = tokens < 256
    mlen = tokens[~lit] - 256
    lfreq = np.bincount(np.where(lit, tokens, 257 + LEN_CODE[np.where(lit, 3, tokens - 256)]), minlength=L_CODES)
    lfreq[END_BLOCK] = 1
    dfreq = np.zeros(D_CODES, np.int64)
    dfreq[0] = mlen.size
    stored_len = int(lit.sum() + mlen.sum())
    st = _State()
    llen, lmax = build_tree(lfreq.tolist(), L_CODES, STATIC_L, png_ref.LEN_EXTRA, 257, 15, st)
    dlen, dmax = build_tree(dfreq.tolist(), D_CODES, STATIC_D, png_ref.DIST_EXTRA, 0, 15, st)
    blfreq = [0] * BL_CODES

    def tally(sym, count):
        blfreq[sym] += 1
    _walk_tree(llen, lmax, tally)
    _walk_tree(dlen, dmax, tally)
    bllen, _ = build_tree(blfreq, BL_CODES, None, EXTRA_BL, 0, 7, st)
    max_blindex = BL_CODES - 1
    while max_blindex >= 3 and bllen[png_ref.CL_ORDER[max_blindex]] == 0:
        max_blindex -= 1
    st.opt_len += 3 * (max_blindex + 1) + 14
    opt_lenb, static_lenb = (st.opt_len + 10) >> 3, (st.static_len + 10) >> 3
    if static_lenb <= opt_lenb:
        opt_lenb = static_lenb
    if stored_len + 4 <= opt_lenb:
        return dict(type=STORED, bits=3 + 32 + 8 * stored_len, stored_len=stored_len, overflow=st.overflow, llen=llen, dlen=dlen, bllen=bllen)
    vals, nbits = [], []
    dyn = dict(overflow=st.overflow, llen=llen, dlen=dlen, bllen=bllen)
    if static_lenb == opt_lenb:
        kind, body = FIXED, st.static_len
        llen, dlen, lmax, dmax = STATIC_L[:L_CODES], STATIC_D, L_CODES - 1, D_CODES - 1
        lcode = gen_codes(STATIC_L, 287)[:L_CODES]
    else:
        kind, body = DYNAMIC, st.opt_len
        lcode = gen_codes(llen, lmax)
        blcode = gen_codes(bllen, BL_CODES - 1)
        vals += [lmax + 1 - 257, dmax + 1 - 1, max_blindex + 1 - 4]
        nbits += [5, 5, 4]
        for rank in range(max_blindex + 1):
            vals.append(bllen[png_ref.CL_ORDER[rank]])
            nbits.append(3)

        def send(sym, count):
            vals.append(blcode[sym])
            nbits.append(bllen[sym])
            if count is not None:
                vals.append(count - (3, 3, 11)[sym - 16])
                nbits.append(EXTRA_BL[sym])
        _walk_tree(llen, lmax, send)
        _walk_tree(dlen, dmax, send)
    dcode = gen_codes(dlen, dmax)
    lcode, llen = np.array(lcode, np.int64), np.array(llen, np.int64)
    # compress_block: per token the literal/length code, the length's extra bits, the distance code (distance 1: code 0, no extra bits)
    lc = LEN_CODE[np.where(lit, 3, tokens - 256)]
    sym = np.where(lit, tokens, 257 + lc)
    ext = np.where(lit, 0, np.array(png_ref.LEN_EXTRA)[lc])
    tv = np.stack([lcode[sym], np.where(lit, 0, tokens - 256 - np.array(png_ref.LEN_BASE)[lc]), np.full(tokens.size, dcode[0])], 1)
    tn = np.stack([llen[sym], ext, np.where(lit, 0, dlen[0])], 1)
    vals = np.concatenate([np.array(vals, np.int64), tv.reshape(-1), [lcode[END_BLOCK]]])
    nbits = np.concatenate([np.array(nbits, np.int64), tn.reshape(-1), [llen[END_BLOCK]]])
    assert 3 + int(nbits.sum()) == 3 + body, "the bits sent differ from the tally (opt_len / static_len)"
    return dict(dyn, type=kind, bits=3 + body, stored_len=stored_len, vals=vals, nbits=nbits)


def _bits_of(vals, nbits):
    """Fields (value, width) -> their bits, each field least significant bit first."""
    vals, nbits = np.asarray(vals, np.int64), np.asarray(nbits, np.int64)
    at = np.arange(int(nbits.sum())) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    return ((np.repeat(vals, nbits) >> at) & 1).astype(np.uint8)


def adler32(raw):
    raw = np.asarray(raw, np.uint8).astype(np.int64)
    n = raw.size
    a = (1 + int(raw.sum())) % 65521
    b = (n + int((raw * (n - np.arange(n))).sum() % 65521)) % 65521 if n < 2 ** 24 else None
    if b is None:                                          # 255 * n * n overflows 63 bits beyond that: reduce the weights first
        b = (n + int((raw * ((n - np.arange(n)) % 65521)).sum() % 65521)) % 65521
    return (b << 16) | a


def deflate(raw, taps=None):
    """The zlib stream of `raw` (uint8) under the rules above."""
    raw = np.asarray(raw, np.uint8)
    tokens = tokenise(raw)
    covered = np.where(tokens < 256, 1, tokens - 256)
    pos = np.concatenate([[0], np.cumsum(covered)])          # the byte each symbol starts at
    n_blocks = tokens.size // BLOCK_SYMBOLS + 1
    bits, blocks, bitoff = [np.array([0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0], np.uint8)], [], []      # 78 01
    at = 16
    for k in range(n_blocks):
        first = k * BLOCK_SYMBOLS
        tk = tokens[first:first + BLOCK_SYMBOLS]
        plan = block_plan(tk)
        last = int(k == n_blocks - 1)
        bitoff.append(at)
        if plan["type"] == STORED:
            assert plan["stored_len"] < 32768 - 262, "a stored block longer than the window keeps (see the docstring)"
            pad = -(at + 3) % 8
            n = plan["stored_len"]
            body = raw[pos[first]:pos[first] + n]
            assert body.size == n
            b = np.concatenate([_bits_of([last, 0], [1, 2]), np.zeros(pad, np.uint8), _bits_of([n, n ^ 0xFFFF], [16, 16]), np.unpackbits(body, bitorder="little")])
        else:
            b = np.concatenate([_bits_of([last, plan["type"]], [1, 2]), _bits_of(plan["vals"], plan["nbits"])])
            assert b.size == plan["bits"]
        blocks.append((plan["type"], first, tk.size, b.size))
        bits.append(b)
        at += b.size
    z = np.packbits(np.concatenate(bits), bitorder="little").tobytes() + struct.pack(">I", adler32(raw))
    if taps is not None:
        taps.update(raw=raw, tokens=tokens, blocks=blocks, bitoff=bitoff, zstream=z)
    return z


def zlib_stream(raw):
    """The judge: what the interpreter's zlib writes at cv2.imwrite's settings."""
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return co.compress(bytes(raw)) + co.flush()


def assemble(w, h, zstream):
    """The file layout: signature | IHDR (8 bit RGB) | one IDAT | IEND."""
    return png_ref.SIGNATURE + png_ref.ihdr(w, h, 8, 2) + png_ref.chunk(b"IDAT", zstream) + png_ref.chunk(b"IEND", b"")


def encode(bgr, filt="sub", taps=None):
    """uint8 [h, w, 3] BGR -> the PNG file (bytes)."""
    h, w = bgr.shape[:2]
    return assemble(w, h, deflate(filtered(bgr, filt), taps))


# ---------------------------------------------------------------- frames the fixtures and the tests share

def make_frame(kind, h, w, seed=0):
    """Small BGR test frames: `noise` (stored blocks), `flat` (one value), `ramp` (smooth gradients: short runs after Sub), `photo` (smooth
    structure and a little noise), `blocks` (flat rectangles: long runs)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), rng.integers(0, 256, 3, dtype=np.uint8), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "ramp":
        return np.stack([(2 * x + y) & 255, (x + 3 * y) & 255, (x * y) & 255], -1).astype(np.uint8)
    if kind == "blocks":
        f = np.zeros((h, w, 3), np.uint8)
        for _ in range(6):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            f[y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = rng.integers(0, 256, 3, dtype=np.uint8)
        return f
    if kind == "photo":
        ch = [128 + 70 * np.sin(x / (23.0 + 7 * c) + c + seed) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 3.1 + c) + rng.normal(0, 2 + c, (h, w))
              for c in range(3)]
        return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def large_frame(seed=11):
    """The 480 x 640 frame the SHA-256 fixture is for, integer arithmetic only (the same on every machine): smooth triangle waves with a little
    noise, flat rectangles top right, noise in the last 80 rows (stored blocks)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:480, 0:640]

    def tri(v, p):
        return np.abs(v % (2 * p) - p)
    f = np.stack([(tri(x + 17 * c, 97 + 13 * c) + tri(y, 61 + 7 * c) + tri(x + 2 * y, 23) // 4 + rng.integers(0, 2 + c, (480, 640))) & 255 for c in range(3)],
                 -1).astype(np.uint8)
    f[:240, 320:] = make_frame("blocks", 240, 320, seed + 1)
    f[400:] = make_frame("noise", 80, 640, seed + 2)
    return f


# ---------------------------------------------------------------- targeted streams (built with frame_for_stream; host and device tests share them)

def literals_then_ones(w, h, n_lit):
    """A Sub-filtered stream of a w x h frame: the first n_lit bytes alternate 2, 3 (every byte a literal symbol, the type bytes 1 included), the
    rest is ONE run of 1s that passes through the type bytes and so crosses rows."""
    p = np.arange(h * (1 + 3 * w))
    s = np.where(p < n_lit, 2 + (p & 1), 1).astype(np.uint8)
    s[::1 + 3 * w] = 1
    return s


def stream_with_symbols(w, h, target):
    """literals_then_ones with exactly `target` symbols."""
    for n_lit in range(target, max(target - 1200, 0), -1):
        s = literals_then_ones(w, h, n_lit)
        if tokenise(s).size == target:
            return s
    raise ValueError("no stream of %d symbols in a %d x %d frame" % (target, w, h))


def spread(counts):
    """{value: count} -> a uint8 sequence with those counts in which no two equal values are neighbours (the most frequent value first on the even
    places, then the odd ones); needs max(count) <= ceil(total / 2)."""
    order = sorted(counts.items(), key=lambda kv: -kv[1])
    flat = np.concatenate([np.full(c, v, np.uint8) for v, c in order])
    out = np.empty(flat.size, np.uint8)
    half = (flat.size + 1) // 2
    out[0::2], out[1::2] = flat[:half], flat[half:]
    assert (out[1:] != out[:-1]).all()
    return out


def one_row_stream(counts):
    """{literal value: count} as the Sub-filtered bytes of a one-row frame: the type byte 1, then spread(counts) with the most frequent value
    raised by up to 2 so that the row is whole pixels -> (stream, w)."""
    counts = dict(counts)
    top = max(counts, key=counts.get)
    counts[top] += -sum(counts.values()) % 3
    s = np.concatenate([[1], spread(counts)]).astype(np.uint8)
    return s, (s.size - 1) // 3


def fibonacci_counts(terms, first_value=10):
    """Literal counts 2, 3, 5, 8, ...: with the type byte and end-of-block (1 each) that is a Fibonacci sequence of `terms` terms, whose Huffman
    tree is a chain `terms` - 1 deep."""
    f = [1, 1]
    while len(f) < terms:
        f.append(f[-1] + f[-2])
    return {first_value + i: c for i, c in enumerate(f[2:])}


def bl_limit_counts():
    """139 literal values with the frequencies max(1, 500 * 1.618^-i): a few Fibonacci-like ones and a long tail of 1s, whose code lengths have
    such counts that the bit-length tree over them needs more than 7 bits before the repair (found by search; the host test asserts it)."""
    f = np.maximum(1, (1.618 ** -np.arange(139.0) * 500).astype(int))
    vals = np.random.default_rng(42).permutation(np.arange(2, 250))[:139]
    return {int(v): int(c) for v, c in zip(vals, f)}


def targeted_frames():
    """name -> BGR frame, each built so that its Sub-filtered stream has one property the encoder can get wrong (the tests assert the property on
    the tokens and blocks of the rule book, then compare bytes).  These are the smallest frames with the property; the symbol-count cases need
    16383 symbols and more, so they are larger than 64 x 64 or one long row."""
    out = {}
    for target in (16382, 16383, 16384, 2 * 16383):                     # 16383 and 2 * 16383: an empty last block
        h = 141 if target < 20000 else 276
        out["symbols_%d" % target] = frame_for_stream(stream_with_symbols(40, h, target), 40, h)
    # a run of 1s that starts at symbol 16381: literal, match 258 | block boundary | match 258 ... (and it crosses rows)
    out["run_across_blocks"] = frame_for_stream(literals_then_ones(40, 143, 16381), 40, 143)
    rows = []
    for R in (259, 260, 261, 262, 4, 3, 2, 1 + 2 * 258 + 3, 1 + 258, 5):  # one run of 7s per row: (R - 1) % 258 in 0, 1, 2, 3 with and without a 258 match
        body = np.concatenate([np.full(R, 7), 2 + (np.arange(600 - R) & 1)])
        rows.append(np.concatenate([[1], body]))
    out["run_remainders"] = frame_for_stream(np.concatenate(rows), 200, len(rows))
    out["flat"] = np.full((7, 9, 3), (13, 200, 77), np.uint8)               # one distance code: the second is forced
    out["no_runs"] = frame_for_stream(literals_then_ones(5, 4, 64), 5, 4)   # no match at all: both distance codes are forced
    out["tiny_1x1"] = np.array([[[3, 1, 2]]], np.uint8)                     # the fixed block wins
    out["tiny_2x2"] = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    rng = np.random.default_rng(9)
    out["noise"] = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)        # stored
    out["noise_two_blocks"] = rng.integers(0, 256, (75, 75, 3), dtype=np.uint8)
    s = literals_then_ones(40, 147, 16383)                                  # 16383 cheap literals (dynamic), then noise (stored, off a byte boundary)
    s[16383:] = rng.integers(0, 256, s.size - 16383, dtype=np.uint8)
    s[::121] = 1
    out["dynamic_then_stored"] = frame_for_stream(s, 40, 147)
    half = np.full((64, 64, 3), 90, np.uint8)                               # half flat, half noise in one block
    half[32:] = rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)
    out["half_flat_half_noise"] = half
    for name, counts in (("fibonacci_16", fibonacci_counts(16)), ("fibonacci_17", fibonacci_counts(17)), ("fibonacci_18", fibonacci_counts(18)),
                         ("bl_limit", bl_limit_counts())):
        s, w = one_row_stream(counts)
        out[name] = frame_for_stream(s, w, 1)
    return out
