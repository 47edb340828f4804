"""Writes tests/golden/png_adam7_cases.npz: Adam7-interlaced PNG files assembled by hand (Pillow reads Adam7 but cannot write it: the pixels are
split into the seven passes, every pass filtered on its own, the lot compressed with zlib and framed: tests/png_adam7_ref.py encode), and the
pixels Pillow (libpng) decodes from the same bytes, converted by the rules cv2.imread asks libpng for and stored BGR (make_golden_png.expected).

    python tools/make_golden_png_adam7.py

Keys as in png_cases.npz: names [n]; file_<name>; bgr_<name> uint8 [h, w, 3] (Pillow's decode); inflated_<name> (zlib.decompress of the IDAT
payloads: the filtered passes one after the other); bad_names [m]; badfile_<name>; badstatus_<name> int32 (the status word the rule book
predicts).  Row r of pass p takes filter type (r + p) % 5, so Average and Paeth meet a pass's first row.  Before anything is written the
generator asserts that the rule book equals Pillow and zlib on every case and that all five filter types were met.
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import png_ref as R  # noqa: E402
import png_adam7_ref as A  # noqa: E402
import make_golden_png as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "png_adam7_cases.npz")
# 1x1: only pass 1 exists; 1x9, 9x1, 2x2, 3x5, 5x3: passes vanish; 8x8: one whole Adam7 cell; 9x17, 17x33: cells crossed; 37x131: pass 7 has 65 rows
SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3), (8, 8), (9, 17), (17, 33), (37, 131)]
TYPES = [("gray1", 1, 0), ("gray2", 2, 0), ("gray4", 4, 0), ("gray8", 8, 0), ("gray16", 16, 0), ("pal1", 1, 3), ("pal2", 2, 3), ("pal4", 4, 3),
         ("pal8", 8, 3), ("rgb8", 8, 2), ("rgb16", 16, 2), ("ga8", 8, 4), ("ga16", 16, 4), ("rgba8", 8, 6), ("rgba16", 16, 6)]
TRNS = R.chunk(b"tRNS", bytes(range(0, 250, 125)))


def build_cases():
    cases = []                                                   # (name, file bytes, filtered scanlines, depth, ctype)

    def add(name, w, h, depth, ctype, seed, **kw):
        rows = G.samples(w, h, R.CHANNELS[ctype], depth, seed)
        if ctype == 3:
            kw.update(palette=G.palette(1 << depth, seed + 100), before_idat=TRNS)      # tRNS present on every palette file (ignored)
        f, raw = A.encode(rows, w, depth, ctype, **kw)
        cases.append((name, f, raw, depth, ctype))

    for i, (w, h) in enumerate(SIZES):                           # every size, RGB 8
        add("rgb8_%dx%d" % (w, h), w, h, 8, 2, 300 + i)
    for i, (name, depth, ctype) in enumerate(TYPES):             # every type at 17 x 33: at depth 1 pass 1 has 3 pixels, a row that ends mid-byte
        if name != "rgb8":
            add("%s_17x33" % name, 17, 33, depth, ctype, 320 + i)
    for i, (name, depth, ctype, w, h) in enumerate([("gray1", 1, 0, 1, 1), ("gray1", 1, 0, 3, 5), ("gray2", 2, 0, 5, 3), ("gray4", 4, 0, 9, 17),
                                                    ("pal1", 1, 3, 9, 1), ("pal2", 2, 3, 2, 2), ("pal4", 4, 3, 1, 9), ("pal4", 4, 3, 8, 8),
                                                    ("gray1", 1, 0, 37, 131), ("rgba16", 16, 6, 37, 131), ("ga8", 8, 4, 5, 3),
                                                    ("rgb16", 16, 2, 3, 5)]):       # sub-byte rows and wide pixels where passes vanish and bands are crossed
        add("%s_%dx%d" % (name, w, h), w, h, depth, ctype, 340 + i)
    add("idat5_rgb8_17x33", 17, 33, 8, 2, 360, split=5)          # many small IDAT chunks
    return cases


def build_malformed():
    out = []
    rows = G.samples(17, 33, 3, 8, 400)
    f, raw = A.encode(rows, 17, 8, 2)
    _, _, z = R.walk(f)
    g = A.geometry(17, 33, 24)
    at = sum(ph * (1 + prb) for _, _, _, _, pw, ph, prb in g[:2]) + 2 * (1 + g[2][6])      # the filter byte of row 2 of pass 3
    bad = bytearray(raw.tobytes())
    assert bad[at] <= 4
    bad[at] = 7
    out.append(("filter_byte_7_in_pass3", R.assemble(17, 33, 8, 2, zlib.compress(bytes(bad), 9), interlace=1)))
    out.append(("idat_cut_to_half", R.assemble(17, 33, 8, 2, z[:len(z) // 2], interlace=1)))
    plain, _ = R.encode(G.samples(17, 33, 1, 2, 401), 17, 2, 0)                             # gray 2: 33 * 6 plain bytes, more when interlaced
    out.append(("plain_stream_under_interlaced_header", R.assemble(17, 33, 2, 0, R.walk(plain)[2], interlace=1)))
    idx = G.samples(17, 33, 1, 8, 402) % 40
    idx[21, 10] = 40                                                                        # an odd row: pass 7
    out.append(("palette_index_past_plte_in_pass7", A.encode(idx, 17, 8, 3, palette=G.palette(40, 403))[0]))
    return out


def main():
    cases, bad = build_cases(), build_malformed()
    reach = R.new_counters()
    arrays = {"names": np.array([c[0] for c in cases]), "bad_names": np.array([b[0] for b in bad])}
    assert len(set(arrays["names"].tolist())) == len(cases)
    for name, f, raw, depth, ctype in cases:
        bgr, inflated, _, st = A.decode_stages(f, reach)
        want = G.expected(f, depth, ctype)
        assert st == 0, (name, st)
        assert np.array_equal(inflated, raw) and inflated.tobytes() == zlib.decompress(R.walk(f)[2]), name
        assert bgr.shape == want.shape and np.array_equal(bgr, want), name
        arrays["file_" + name] = np.frombuffer(f, np.uint8)
        arrays["bgr_" + name] = want
        arrays["inflated_" + name] = inflated
    assert all(reach["filters"]), reach
    want_status = {"filter_byte_7_in_pass3": R.ST_BAD_FILTER, "idat_cut_to_half": R.ST_INPUT_EXHAUSTED,
                   # fewer bytes than the seven passes hold, and pixel bytes of the plain rows standing where the passes' filter bytes are read
                   "plain_stream_under_interlaced_header": R.ST_TOO_FEW_BYTES | R.ST_BAD_FILTER,
                   "palette_index_past_plte_in_pass7": R.ST_BAD_PALETTE_INDEX}
    for name, f in bad:
        st = A.decode_stages(f)[3]
        assert st == want_status[name], (name, st)
        arrays["badfile_" + name] = np.frombuffer(f, np.uint8)
        arrays["badstatus_" + name] = np.int32(st)
    np.savez_compressed(OUT, **arrays)
    print("%d cases + %d malformed -> %s (%d bytes); filters %s" % (len(cases), len(bad), OUT, os.path.getsize(OUT), reach["filters"]))


if __name__ == "__main__":
    main()
