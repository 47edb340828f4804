"""The rule book of the TIFF encoder (maf-yolo_amd/tiff_encode.py, csrc/tiff_encode.hip) in plain Python and numpy.  No GPU, no Pillow.

What the device computes, restated serially; tests/test_tiff_encode_host.py holds it to Pillow / libtiff 4.7.1 strip by strip:
  * cv2_rows_per_strip(w, h)   clamp(8192 // (3 * w), 1, h): the division first, so a row wider than 8192 bytes is a strip of its own;
  * differenced(bgr, predictor)  B, G, R -> R, G, B, then per row and channel d[x] = p[x] - p[x - 1] mod 256 with d[0] = p[0] (Predictor 2);
                               predictor=False: the plain RGB rows;
  * lzw(data, taps)            libtiff's LZW encoder as a rule over the codes it emits (its hash table is an implementation detail): MSB-first
                               codes of 9 to 12 bits, Clear 256 in front, EOI 257 behind, "early change" widths, a Clear when the table is full
                               (the next free entry would be 4094) and a Clear when, at a checkpoint every 10000 input bytes, the compression
                               ratio (input bytes << 8) // output bits has not grown.  All state is fresh at the start of a strip.
                               taps: codes (with the Clears and the EOI), clears (indices into codes), widths, free_at_end (the next free
                               entry when the last data code went out), ratio_records / ratio_resets (checkpoints that only recorded / reset);
  * assemble / encode          the file: II*\\0 and the IFD offset, the strips back to back from byte 8, a zero byte where their end is odd,
                               the BitsPerSample, StripOffsets and StripByteCounts arrays (the last two inline for a single strip), then the
                               IFD of eleven entries (ten without the predictor) in ascending tag order and a next-IFD of 0.
A strip is under 2^23 bytes (the encoder refuses more), so libtiff's second ratio formula for huge counts is never reached.
"""
import struct

import numpy as np

from png_encode_ref import make_frame, large_frame  # noqa: F401  (the frames the encoders' fixtures share)

CLEAR, EOI, FIRST, TABLE_FULL, CHECK_GAP = 256, 257, 258, 4094, 10000
SHORT, LONG = 3, 4
MAX_STRIP = 1 << 23


def cv2_rows_per_strip(w, h):
    return min(max(8192 // (3 * w), 1), h)


def differenced(bgr, predictor=True):
    """uint8 [h, w, 3] BGR -> uint8 [h, 3 * w]: the bytes the LZW stage reads."""
    rgb = np.ascontiguousarray(bgr[:, :, ::-1])
    if predictor:
        d = rgb.copy()
        d[:, 1:] = rgb[:, 1:] - rgb[:, :-1]              # uint8 arithmetic wraps mod 256
        rgb = d
    return rgb.reshape(bgr.shape[0], 3 * bgr.shape[1])


def code_width(k):
    """The width of the k-th code behind a Clear (k = 0: the first); the Clear that ends the run is written at this width too."""
    return 9 + (k >= 254) + (k >= 766) + (k >= 1790)


def lzw(data, taps=None):
    """One strip's bytes -> its LZW stream (bytes), by the rule of the module docstring."""
    data = bytes(data)
    assert 0 < len(data) < MAX_STRIP
    codes, widths, clears, records, resets = [], [], [], [], []
    st = dict(nbits=9, free=FIRST, incount=0, outcount=0, ratio=0, checkpoint=CHECK_GAP)
    table = {}

    def put(c):
        codes.append(c)
        widths.append(st["nbits"])
        st["outcount"] += st["nbits"]

    def reset():
        table.clear()
        st["free"], st["ratio"], st["incount"], st["outcount"] = FIRST, 0, 0, 0
        clears.append(len(codes))
        put(CLEAR)                                      # at the old width
        st["nbits"] = 9

    clears.append(0)
    put(CLEAR)
    ent = data[0]
    st["incount"] = 1
    for c in data[1:]:
        st["incount"] += 1
        nxt = table.get((ent, c))
        if nxt is not None:
            ent = nxt
            continue
        put(ent)
        table[(ent, c)] = st["free"]
        ent = c
        st["free"] += 1
        if st["free"] == TABLE_FULL:
            reset()
        elif st["free"] > (1 << st["nbits"]) - 1:
            st["nbits"] += 1
        elif st["incount"] >= st["checkpoint"]:
            st["checkpoint"] = st["incount"] + CHECK_GAP           # never reset by reset()
            rat = (st["incount"] << 8) // st["outcount"]
            if rat <= st["ratio"]:
                resets.append(len(codes))
                reset()
            else:
                records.append(len(codes))
                st["ratio"] = rat
    put(ent)
    free_at_end = st["free"]
    st["free"] += 1
    if st["free"] == TABLE_FULL:
        clears.append(len(codes))
        put(CLEAR)
        st["nbits"] = 9
    elif st["free"] > (1 << st["nbits"]) - 1:
        st["nbits"] += 1
    put(EOI)
    bits = sum(widths)
    acc = 0
    for c, n in zip(codes, widths):
        acc = (acc << n) | c
    out = (acc << (-bits % 8)).to_bytes((bits + 7) // 8, "big")
    if taps is not None:
        taps.update(codes=codes, widths=widths, clears=clears, bits=bits, free_at_end=free_at_end, ratio_records=records, ratio_resets=resets)
    return out


def strips_of(bgr, rows_per_strip=None, predictor=True, taps=None):
    """-> (rows per strip, [the LZW stream of every strip]).  taps: raw (the differenced bytes, uint8 [h * 3 * w]) and strips, a list of lzw's taps."""
    h, w = bgr.shape[:2]
    rps = cv2_rows_per_strip(w, h) if rows_per_strip is None else int(rows_per_strip)
    assert 1 <= rps <= h
    rows = differenced(bgr, predictor)
    out, per = [], []
    for y in range(0, h, rps):
        t = {}
        out.append(lzw(rows[y:y + rps].tobytes(), t))
        per.append(t)
    if taps is not None:
        taps.update(raw=rows.reshape(-1), strips=per, rows_per_strip=rps)
    return rps, out


def assemble(w, h, rows_per_strip, strips, predictor=True, taps=None):
    """The file around the strips."""
    n = len(strips)
    offsets, at = [], 8
    for s in strips:
        offsets.append(at)
        at += len(s)
    body = b"".join(strips) + b"\0" * (at & 1)
    at += at & 1
    bits_at = at
    arrays = struct.pack("<3H", 8, 8, 8)
    if n > 1:
        off_at, cnt_at = bits_at + 6, bits_at + 6 + 4 * n
        arrays += struct.pack("<%dI" % n, *offsets) + struct.pack("<%dI" % n, *(len(s) for s in strips))
    else:
        off_at, cnt_at = offsets[0], len(strips[0])          # inline values
    ifd_at = bits_at + len(arrays)
    entries = [(256, SHORT, 1, w), (257, SHORT, 1, h), (258, SHORT, 3, bits_at), (259, SHORT, 1, 5), (262, SHORT, 1, 2), (273, LONG, n, off_at),
               (277, SHORT, 1, 3), (278, SHORT, 1, rows_per_strip), (279, LONG, n, cnt_at), (284, SHORT, 1, 1)]
    if predictor:
        entries.append((317, SHORT, 1, 2))
    ifd = struct.pack("<H", len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + struct.pack("<I", 0)
    if taps is not None:
        taps.update(offsets=offsets, lengths=[len(s) for s in strips], ifd_at=ifd_at)
    return b"II*\0" + struct.pack("<I", ifd_at) + body + arrays + ifd


def encode(bgr, rows_per_strip=None, predictor=True, taps=None):
    """uint8 [h, w, 3] BGR -> the TIFF file (bytes)."""
    h, w = bgr.shape[:2]
    rps, strips = strips_of(bgr, rows_per_strip, predictor, taps)
    return assemble(w, h, rps, strips, predictor, taps)


def file_strips(data):
    """A file's strips as it names them -> (tags of the first IFD, [bytes per strip])."""
    import tiff_ref
    _, t = tiff_ref.read_ifd(data)
    return t, [bytes(data[o:o + n]) for o, n in zip(t[273], t[279])]


# ---------------------------------------------------------------- targeted frames (host and device tests share them)

def frame_for_rows(rows, w):
    """The BGR frame whose differenced rows are `rows` (uint8 [h, 3 * w]): the running sum per channel, reversed."""
    rgb = (np.cumsum(np.asarray(rows, np.uint8).reshape(-1, w, 3).astype(np.int64), axis=1) & 255).astype(np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _noise_row(seed, pixels):
    return np.random.default_rng(seed).integers(0, 256, (1, 3 * pixels), dtype=np.uint8)


def _search(build, wanted, limit=4000):
    """The first candidate build(i), i = 0, 1, ..., whose LZW taps satisfy `wanted`."""
    for i in range(limit):
        rows = build(i)
        t = {}
        lzw(rows.tobytes(), t)
        if wanted(t):
            return rows
    raise AssertionError("no candidate found")


def smooth_row(pixels, seed=0):
    x = np.arange(pixels)
    return np.stack([(x // 3 + seed) & 255, (x // 5 + 2 * seed) & 255, (x // 7) & 255], -1).astype(np.uint8)[None, :, ::-1]


def two_part_row(pixels=10000, flat=3400, seed=0):
    """One row whose differenced bytes are `flat` pixels of zeros, then bytes drawn from {0, 1}: compresses well at first, then worse."""
    rng = np.random.default_rng(seed)
    d = np.zeros((1, 3 * pixels), np.uint8)
    d[0, 3 * flat:] = rng.integers(0, 2, 3 * (pixels - flat), dtype=np.uint8)
    return d


def _noise_with(seed0, pixels0, span, wanted):
    """A one-row noise strip of pixels0 .. pixels0 + span - 1 pixels (seeds seed0, seed0 + 1, ... in turn) whose LZW taps satisfy `wanted`."""
    return _search(lambda i: _noise_row(seed0 + i // span, pixels0 + i % span), wanted)


def table_full_resets(t):
    """Indices (into the codes) of the Clears written because the table was full, the one behind the last data code included."""
    return [c for c in t["clears"][1:] if c not in t["ratio_resets"]]


def targeted_frames():
    """name -> BGR frame, every one a single row (so a single strip under the cv2 rule as well).  What each is for is asserted from the
    rule book's taps in tests/test_tiff_encode_host.py."""
    rows = {}
    for free in (511, 1023, 2047):                       # the last data code leaves with the next free entry at `free`: the EOI is a bit wider
        rows["eoi_bump_%d" % free] = _noise_with(free, (free - 257) // 3, 120, lambda t: t["free_at_end"] == free and len(t["clears"]) == 1)
    rows["ends_as_table_fills"] = _noise_with(7, 3836 // 3, 400, lambda t: t["free_at_end"] == TABLE_FULL - 1 and t["codes"][-2:] == [CLEAR, EOI])
    rows["one_table_full_reset"] = _noise_row(21, 2000)                                  # noise fills the table within about 4000 bytes
    rows["two_table_full_resets"] = _noise_row(22, 2731)                                 # 8193 bytes of noise
    rows["ratio_records"] = differenced(smooth_row(4000))
    rows["ratio_resets"] = two_part_row()
    rows["ends_on_a_byte"] = _noise_with(31, 1, 40, lambda t: t["bits"] % 8 == 0)
    rows["needs_padding"] = _noise_with(32, 5, 40, lambda t: t["bits"] % 8 == 3)
    rows["one_pixel"] = _noise_row(33, 1)
    return {name: frame_for_rows(r, r.shape[1] // 3) for name, r in rows.items()}
