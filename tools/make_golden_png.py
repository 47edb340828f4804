"""Writes tests/golden/png_cases.npz: PNG files written by hand (chunks + zlib.compressobj, tests/png_ref.py encode), so that every decoder
path is reached on purpose (Pillow's writer picks filters and strategies itself), and the pixels Pillow (libpng + zlib) decodes from the same
bytes, converted by the rules cv2.imread asks libpng for (maf-yolo_amd/png.py) and stored BGR.

    python tools/make_golden_png.py

Keys: names [n]; file_<name> uint8 (the PNG bytes); bgr_<name> uint8 [h, w, 3] (expected frame: Pillow's decode); inflated_<name> uint8
[h * (1 + rowbytes)] (the filtered scanlines: zlib.decompress of the IDAT payloads); bad_names [m]; badfile_<name>; badstatus_<name> int32 (the
status word tests/png_ref.py predicts for the malformed file).  Before anything is written the generator asserts that png_ref equals Pillow
and zlib on every case, and, through png_ref's counters, that the set reaches: all three block types, a match of length 258, a match with
distance < length, a match at distance >= 32 000, a code longer than the first-level lookup, all five filter types.
"""
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "png_cases.npz")
CYCLE = (0, 1, 2, 3, 4)


def samples(w, h, ch, depth, seed):
    """Packed rows uint8 [h, rowbytes] of a picture with smooth parts (matches), flat parts (long matches) and noisy parts (literals)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = np.stack([(x * (3 + c) + y * (5 - c) + 40 * c) for c in range(ch)], -1).astype(np.int64)
    v += rng.integers(0, 24, (h, w, ch)) * ((x + y) % 7 < 3)[:, :, None]
    v[h // 3:h // 2] = v[h // 3:h // 3 + 1]                      # a band of equal rows
    top = 1 << depth
    if depth == 16:
        v = (v * 257 + rng.integers(0, 256, (h, w, ch))) % top
        b = np.stack([v >> 8, v & 255], -1).astype(np.uint8)     # big-endian
        return b.reshape(h, w * ch * 2)
    v = (v % top if depth == 8 else (v // 3) % top).astype(np.uint8)
    if depth == 8:
        return v.reshape(h, w * ch)
    bits = ((v.reshape(h, w, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, w * depth)
    return np.packbits(bits, axis=1)                             # MSB first, the last byte padded with zeros


def palette(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def expected(data, depth, ctype):
    """Pillow's decode of the file under the conversion rules -> uint8 [h, w, 3] BGR."""
    im = Image.open(io.BytesIO(data))
    im.load()
    if im.mode in ("I;16", "I;16B", "I"):                        # 16-bit gray arrives as raw values: the high byte
        g = (np.asarray(im).astype(np.int64) >> 8).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))
    if im.mode == "P":
        im.info.pop("transparency", None)
    rgb = np.asarray(im.convert("RGBA" if im.mode in ("LA", "RGBA", "PA") else "RGB"))[:, :, :3]     # alpha dropped, not composited
    return np.ascontiguousarray(rgb[:, :, ::-1])


def build_cases():
    cases = []                                                   # (name, file bytes, filtered scanlines, depth, ctype)

    def add(name, w, h, depth, ctype, seed, **kw):
        rows = kw.pop("rows", None)
        if rows is None:
            rows = samples(w, h, R.CHANNELS[ctype], depth, seed)
        if ctype == 3 and "palette" not in kw:
            kw["palette"] = palette(1 << depth, seed + 100)
        f, raw = R.encode(rows, w, depth, ctype, **kw)
        cases.append((name, f, raw, depth, ctype))

    for i, (w, h) in enumerate([(1, 1), (1, 7), (7, 1), (3, 5), (17, 33), (64, 48)]):            # sizes, RGB 8, dynamic, filters cycled
        add("rgb8_%dx%d" % (w, h), w, h, 8, 2, i)
    for name, depth, ctype, w, h in [("rgb16", 16, 2, 17, 33), ("rgba8", 8, 6, 17, 33), ("rgba16", 16, 6, 17, 33), ("gray8", 8, 0, 17, 33),
                                     ("gray16", 16, 0, 17, 33), ("ga8", 8, 4, 17, 33), ("ga16", 16, 4, 17, 33), ("gray1", 1, 0, 17, 33),
                                     ("gray2", 2, 0, 17, 33), ("gray4", 4, 0, 17, 33), ("gray1", 1, 0, 3, 5), ("gray2", 2, 0, 5, 7),
                                     ("gray4", 4, 0, 3, 5), ("pal1", 1, 3, 17, 33), ("pal2", 2, 3, 5, 7), ("pal4", 4, 3, 17, 33),
                                     ("pal4", 4, 3, 3, 5), ("pal8", 8, 3, 17, 33)]:
        add("%s_%dx%d" % (name, w, h), w, h, depth, ctype, 20 + len(cases))
    # tRNS on a palette, a gray and an RGB file; gAMA / pHYs / tEXt in front of the IDAT chunks (all skipped); a PLTE shorter than 2^depth
    anc = R.chunk(b"gAMA", (45455).to_bytes(4, "big")) + R.chunk(b"pHYs", bytes(9)) + R.chunk(b"tEXt", b"Comment\x00made by hand")
    add("pal8_trns_17x33", 17, 33, 8, 3, 50, before_idat=R.chunk(b"tRNS", bytes(range(0, 250, 10))) + anc)
    add("gray8_trns_17x33", 17, 33, 8, 0, 51, before_idat=R.chunk(b"tRNS", b"\x00\x10"))
    add("rgb8_trns_anc_17x33", 17, 33, 8, 2, 52, before_idat=anc + R.chunk(b"tRNS", b"\x00\x10\x00\x20\x00\x30"))
    add("pal4_short_plte_17x33", 17, 33, 4, 3, 53, rows=samples(17, 33, 1, 4, 53) & 0x77, palette=palette(8, 153))
    for ft in range(5):                                          # every filter type on the first row and on all later rows
        add("rgb8_filter%d_17x33" % ft, 17, 33, 8, 2, 60 + ft, filters=(ft,))
        add("rgba16_filter%d_5x7" % ft, 5, 7, 16, 6, 70 + ft, filters=(ft,))
    add("gray2_filter_cycle_from4_17x33", 17, 33, 2, 0, 80, filters=(4, 3, 2, 1, 0))
    # deflate
    add("stored_rgb8_64x48", 64, 48, 8, 2, 90, level=0)
    y, x = np.mgrid[0:100, 0:128 * 8]
    add("stored_straddle_rgba16_128x100", 128, 100, 16, 6, 0, rows=((x // 8 + y) & 255).astype(np.uint8), level=0, filters=(0,))   # 102 500 bytes: blocks of 65 535
    add("fixed_rgb8_64x48", 64, 48, 8, 2, 91, strategy=zlib.Z_FIXED)
    add("huffman_only_rgb8_64x48", 64, 48, 8, 2, 92, strategy=zlib.Z_HUFFMAN_ONLY)
    add("rle_rgb8_64x48", 64, 48, 8, 2, 93, strategy=zlib.Z_RLE)
    add("memlevel1_rgb8_64x48", 64, 48, 8, 2, 94, mem_level=1)
    add("memlevel1_noise_rgb8_64x48", 64, 48, 8, 2, 0, rows=np.random.default_rng(95).integers(0, 256, (48, 192), dtype=np.uint8), mem_level=1, filters=(0,))
    add("fullflush_rgb8_64x48", 64, 48, 8, 2, 96, flush_at=4000)
    add("idat1_rgb8_17x33", 17, 33, 8, 2, 97, split=1)
    add("idat7_rgb8_64x48", 64, 48, 8, 2, 98, split=7)
    add("flat_gray8_64x48", 64, 48, 8, 0, 0, rows=np.full((48, 64), 200, np.uint8), filters=(0,))       # matches of length 258 at distance 1
    # 128 x 100 RGB 8: 38 500 scanline bytes, more than the 32 KiB window; rows 84 .. 93 repeat rows 0 .. 9 (noise, filter 0) at distance 84 * 385 = 32 340
    rng = np.random.default_rng(99)
    big = samples(128, 100, 3, 8, 99)
    big[10:84] = (big[10:84].astype(np.int64) + rng.integers(0, 64, (74, 384))).astype(np.uint8)
    big[0:10] = rng.integers(0, 256, (10, 384), dtype=np.uint8)
    big[84:94] = big[0:10]
    add("window_rgb8_128x100", 128, 100, 8, 2, 0, rows=big, filters=(0,))
    return cases


def build_malformed():
    out = []
    rows = samples(17, 33, 3, 8, 200)
    f, _ = R.encode(rows, 17, 8, 2)
    _, _, z = R.walk(f)
    out.append(("idat_cut_to_half", R.assemble(17, 33, 8, 2, z[:len(z) // 2])))
    # one hand-assembled fixed-Huffman block for a 1 x 1 gray image: BFINAL 1, BTYPE 01, literal 0 (code 00110000), length 3 (symbol 257: 0000001),
    # distance symbol 4 (00100) + extra bit 0 = distance 5, with one byte produced
    bits = "1" + "10" + "00110000" + "0000001" + "00100" + "0" + "0000000"
    bits += "0" * (-len(bits) % 8)
    body = bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8))
    out.append(("distance_before_start", R.assemble(1, 1, 8, 0, b"\x78\x01" + body + bytes(4))))
    raw = bytearray(R.filter_rows(rows, CYCLE, 3).tobytes())
    raw[5 * (1 + 51)] = 7
    out.append(("filter_byte_7", R.assemble(17, 33, 8, 2, zlib.compress(bytes(raw), 9))))
    idx = samples(17, 33, 1, 8, 201) % 40
    idx[20, 11] = 40
    out.append(("palette_index_past_plte", R.encode(idx, 17, 8, 3, palette=palette(40, 202))[0]))
    return out


def main():
    cases, bad = build_cases(), build_malformed()
    reach = R.new_counters()
    arrays = {"names": np.array([c[0] for c in cases]), "bad_names": np.array([b[0] for b in bad])}
    assert len(set(arrays["names"].tolist())) == len(cases)
    for name, f, raw, depth, ctype in cases:
        bgr, inflated, _, st = R.decode_stages(f, reach)
        want = expected(f, depth, ctype)
        _, _, z = R.walk(f)
        assert st == 0, (name, st)
        assert np.array_equal(inflated, raw) and inflated.tobytes() == zlib.decompress(z), name
        assert bgr.shape == want.shape and np.array_equal(bgr, want), name
        arrays["file_" + name] = np.frombuffer(f, np.uint8)
        arrays["bgr_" + name] = want
        arrays["inflated_" + name] = inflated
    assert reach["stored"] and reach["fixed"] and reach["dynamic"], reach
    assert reach["max_match"] == 258 and reach["overlap"] and reach["max_distance"] >= 32000 and reach["long_code"], reach
    assert all(reach["filters"]), reach
    want_status = {"idat_cut_to_half": R.ST_INPUT_EXHAUSTED, "distance_before_start": R.ST_DISTANCE_TOO_FAR, "filter_byte_7": R.ST_BAD_FILTER,
                   "palette_index_past_plte": R.ST_BAD_PALETTE_INDEX}
    for name, f in bad:
        st = R.decode_stages(f)[3]
        assert st == want_status[name], (name, st)
        arrays["badfile_" + name] = np.frombuffer(f, np.uint8)
        arrays["badstatus_" + name] = np.int32(st)
    np.savez_compressed(OUT, **arrays)
    print("%d cases + %d malformed -> %s (%d bytes); reached %s" % (len(cases), len(bad), OUT, os.path.getsize(OUT), reach))


if __name__ == "__main__":
    main()
