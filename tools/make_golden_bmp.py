"""Writes tests/golden/bmp_cases.npz: the BMP and MPO fixtures of tests/test_bmp_host.py, tests/test_gpu_bmp.py and tests/test_gpu_mpo.py.

    python tools/make_golden_bmp.py

Every good BMP case is a file assembled by hand (tests/bmp_ref.py; Pillow cannot write RLE, 1 / 4-bit rows of any width, or most header kinds),
stored as file_<name> beside bgr_<name>: PILLOW's pixels, reversed to BGR, and judge_<name>: "direct" where Pillow decoded that very file,
"rewrite" where the file holds a construct Pillow 12.2 reads differently from the rule (bmp_ref.departs) and Pillow decoded bmp_ref.rewrite
of it.  The tool asserts that the rule book (bmp_ref.decode_stages) gives the same pixels with status 0 — for a rewritten case on the file
and on its rewrite — before it stores anything, so a fixture is a file on which Pillow and the rule book agree.  The malformed files are
stored as badfile_<name> with badstatus_<name>, the status word the rule book predicts; they are never compared with Pillow.  The MPO files
(mpofile_<name>, mpobgr_<name>) are written by Pillow with a second frame of another size; the pixels are Pillow's decode of the first frame.
Synthetic pictures only.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bmp_ref as R  # noqa: E402


def cases():
    """-> ([(name, file bytes)], [(name, file bytes)]): the good and the malformed files."""
    rng = np.random.default_rng(11)
    good, bad = [], []
    pal2, pal16, pal256 = (rng.integers(0, 256, (k, 3), dtype=np.uint8) for k in (2, 16, 256))
    # uncompressed rows: every width at which the packing or the 4-byte padding changes
    for w in (1, 7, 8, 9, 31, 32, 33):
        good.append(("bi1_w%d" % w, R.assemble(w, 3, 1, R.pack_rows(rng.integers(0, 2, (3, w)), 1), palette=pal2)))
    for w in (1, 2, 3, 7, 8, 9):
        good.append(("bi4_w%d" % w, R.assemble(w, 3, 4, R.pack_rows(rng.integers(0, 16, (3, w)), 4), palette=pal16)))
    for w in (1, 2, 3, 4, 5):
        good.append(("bi8_w%d" % w, R.assemble(w, 3, 8, R.pack_rows(rng.integers(0, 256, (3, w)), 8), palette=pal256)))
    for w in (1, 2, 3, 4, 5):                                  # row padding 3, 2, 1, 0, 3
        good.append(("bgr24_w%d" % w, R.assemble(w, 3, 24, R.pack_rows(rng.integers(0, 256, (3, w, 3)), 24))))
    good.append(("bgr24_16x5_rows_of_48", R.assemble(16, 5, 24, R.pack_rows(rng.integers(0, 256, (5, 16, 3)), 24))))      # 16-byte aligned rows
    good.append(("bgr24_12x4_rows_of_36", R.assemble(12, 4, 24, R.pack_rows(rng.integers(0, 256, (4, 12, 3)), 24))))      # 4-byte aligned rows
    good.append(("bgr24_13x3_top_down", R.assemble(13, 3, 24, R.pack_rows(rng.integers(0, 256, (3, 13, 3)), 24, True), top_down=True)))
    px32 = rng.integers(1, 256, (4, 5, 4))                     # non-zero 4th bytes
    good.append(("bgrx32_plain", R.assemble(5, 4, 32, R.pack_rows(px32, 32))))
    good.append(("bgrx32_bitfields_header40", R.assemble(5, 4, 32, R.pack_rows(px32, 32), compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF))))
    good.append(("bgra32_bitfields_header108_alpha", R.assemble(5, 4, 32, R.pack_rows(px32, 32), header=108, compression=R.BITFIELDS,
                                                                masks=(0xFF0000, 0xFF00, 0xFF), alpha=0xFF000000)))
    good.append(("bgrx32_bitfields_header52", R.assemble(5, 4, 32, R.pack_rows(px32, 32), header=52, compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF))))
    # shape and headers
    i8 = rng.integers(0, 256, (6, 11))
    good.append(("bi8_h1", R.assemble(11, 1, 8, R.pack_rows(i8[:1], 8), palette=pal256)))
    good.append(("bi4_top_down", R.assemble(11, 6, 4, R.pack_rows(i8 & 15, 4, True), palette=pal16, top_down=True)))
    good.append(("bi8_header12_os2", R.assemble(11, 6, 8, R.pack_rows(i8, 8), header=12, palette=pal256)))
    good.append(("bi1_header12_os2", R.assemble(11, 6, 1, R.pack_rows(i8 & 1, 1), header=12, palette=pal2)))
    good.append(("bi8_header52", R.assemble(11, 6, 8, R.pack_rows(i8, 8), header=52, palette=pal256)))
    good.append(("bgr24_header56", R.assemble(7, 3, 24, R.pack_rows(rng.integers(0, 256, (3, 7, 3)), 24), header=56)))
    good.append(("bi4_header64", R.assemble(11, 6, 4, R.pack_rows(i8 & 15, 4), header=64, palette=pal16)))
    good.append(("bi1_header108", R.assemble(11, 6, 1, R.pack_rows(i8 & 1, 1), header=108, palette=pal2)))
    good.append(("bgr24_header124", R.assemble(7, 3, 24, R.pack_rows(rng.integers(0, 256, (3, 7, 3)), 24), header=124)))
    # palettes
    good.append(("bi8_colors2_out_of_palette", R.assemble(11, 6, 8, R.pack_rows(i8 % 5, 8), palette=pal2)))
    good.append(("bi4_colors5_out_of_palette", R.assemble(11, 6, 4, R.pack_rows(i8 & 15, 4), palette=pal16[:5])))
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    good.append(("bi8_gray_palette", R.assemble(11, 6, 8, R.pack_rows(i8, 8), palette=gray)))
    good.append(("bi1_black_white", R.assemble(11, 6, 1, R.pack_rows(i8 & 1, 1), palette=np.array([[0, 0, 0], [255, 255, 255]], np.uint8))))
    good.append(("bi8_gap_before_data", R.assemble(11, 6, 8, R.pack_rows(i8, 8), palette=pal256, gap=10)))
    good.append(("bgr24_gap_before_data", R.assemble(7, 3, 24, R.pack_rows(rng.integers(0, 256, (3, 7, 3)), 24), gap=6)))
    # RLE
    for rle4 in (False, True):
        k = "rle4_" if rle4 else "rle8_"
        pal = pal16 if rle4 else pal256
        top = 16 if rle4 else 256
        def v():                                               # the byte of an encoded run (RLE4: two nibbles)
            return int(rng.integers(1, 256 if rle4 else top))

        def px(n):
            return [int(t) for t in rng.integers(0, top, n)]

        good.append((k + "runs_of_1_and_255", R.rle_file(260, 2, [("run", 255, v()), ("run", 1, v()), ("run", 4, v()), ("eol",),
                                                                   ("run", 1, v()), ("run", 255, v()), ("run", 4, v()), ("eob",)], rle4, pal)))
        good.append((k + "absolute_3_4_5", R.rle_file(12, 2, [("abs", px(3)), ("abs", px(4)), ("abs", px(5)), ("eol",),
                                                               ("abs", px(5)), ("abs", px(4)), ("abs", px(3)), ("eob",)], rle4, pal)))
        good.append((k + "absolute_254_255_longer_than_a_window", R.rle_file(260, 2, [("abs", px(254)), ("run", 6, v()), ("eol",),
                                                                                       ("run", 5, v()), ("abs", px(255)), ("eob",)], rle4, pal)))
        good.append((k + "delta_mid_row_and_at_row_end", R.rle_file(10, 5, [("run", 3, v()), ("delta", 2, 0), ("run", 5, v()), ("delta", 0, 1), ("eol",),
                                                                             ("run", 4, v()), ("delta", 3, 1), ("run", 3, v()), ("eol",),
                                                                             ("run", 10, v()), ("eob",)], rle4, pal)))
        good.append((k + "empty_row_eol", R.rle_file(6, 4, [("run", 6, v()), ("eol",), ("eol",), ("abs", px(6)), ("eol",), ("run", 6, v()), ("eob",)], rle4, pal)))
        good.append((k + "early_eob", R.rle_file(6, 4, [("run", 6, v()), ("eol",), ("run", 3, v()), ("eob",)], rle4, pal)))
        good.append((k + "early_eob_on_an_empty_row", R.rle_file(6, 4, [("run", 6, v()), ("eol",), ("eob",)], rle4, pal)))
        good.append((k + "data_after_eob", R.rle_file(6, 2, [("run", 6, v()), ("eol",), ("abs", px(6)), ("eob",), ("raw", bytes([3, 7, 0, 9, 1, 2, 3, 0xFF, 0xFF]))], rle4, pal)))
        plane = rng.integers(0, top, (5, 9))
        plane[2, 1:8] = 3
        good.append((k + "no_eol_before_eob", R.rle_file(9, 5, R.rle_records(plane, rle4), rle4, pal)))
        good.append((k + "eol_before_eob", R.rle_file(9, 5, R.rle_records(plane, rle4, eol_last=True), rle4, pal)))
        good.append((k + "full_image_without_eob", R.rle_file(9, 5, R.rle_records(plane, rle4)[:-1], rle4, pal)))
        # the device fetches windows of 128 bytes: 63 records of 2 bytes put the next one on the window's last lane
        ones = [("run", 1, v()) for _ in range(63)]
        good.append((k + "delta_operands_straddle_a_window", R.rle_file(70, 2, ones + [("delta", 2, 0), ("run", 5, v()), ("eol",), ("run", 70, v()), ("eob",)], rle4, pal)))
        good.append((k + "absolute_header_on_the_last_lane", R.rle_file(70, 2, ones + [("abs", px(6)), ("run", 1, v()), ("eol",), ("abs", px(70)), ("eob",)], rle4, pal)))
        n_abs = 80 if rle4 else 40                             # the payload begins at byte 102 and ends behind byte 128
        good.append((k + "absolute_payload_straddles_a_window", R.rle_file(50 + n_abs, 2, ones[:50] + [("abs", px(n_abs)), ("eol",), ("run", 50 + n_abs, v()), ("eob",)],
                                                                           rle4, pal)))
        noise = rng.integers(0, top, (50, 70))
        noise[10:14, 5:60] = noise[10:14, 5:6]                 # some runs among the absolute records
        noise[30:34, 20:31] = 0
        good.append((k + "noise_70x50", R.rle_file(70, 50, R.rle_records(noise, rle4), rle4, pal)))
        good.append((k + "noise_70x50_short_absolute_runs", R.rle_file(70, 50, R.rle_records(noise, rle4, abs_max=6), rle4, pal)))
        good.append((k + "single_colour_40x6", R.rle_file(40, 6, R.rle_records(np.full((6, 40), 5), rle4), rle4, pal)))
        good.append((k + "1x1", R.rle_file(1, 1, [("run", 1, v()), ("eob",)], rle4, pal)))
        good.append((k + "colors3_out_of_palette", R.rle_file(9, 5, R.rle_records(plane, rle4), rle4, pal[:3])))
    good.append(("rle4_noise_odd_absolute_runs", R.rle_file(23, 7, [r for y in range(7) for r in (("abs", [int(t) for t in rng.integers(0, 16, 23)]), ("eol",))][:-1] + [("eob",)],
                                                            True, pal16)))
    # malformed: status bits, never Pillow; records behind the fault would write if the walk went on
    tail = [("eol",), ("run", 4, 0x77), ("eob",)]
    bad.append(("rle8_ends_without_eob", R.rle_file(8, 3, [("run", 8, 9), ("eol",), ("run", 5, 7)], False, pal256)))
    bad.append(("rle8_absolute_payload_cut", R.rle_file(8, 3, [("run", 8, 9), ("eol",), ("raw", bytes([0, 6, 1, 2, 3]))], False, pal256)))
    bad.append(("rle4_delta_operands_cut", R.rle_file(8, 3, [("run", 8, 0x12), ("eol",), ("raw", bytes([0, 2, 1]))], True, pal16)))
    bad.append(("rle8_run_past_row", R.rle_file(8, 3, [("run", 5, 9), ("run", 6, 200)] + tail, False, pal256)))
    bad.append(("rle4_absolute_run_past_row", R.rle_file(8, 3, [("run", 5, 0x12), ("abs", [1, 2, 3, 4, 5, 6])] + tail, True, pal16)))
    bad.append(("rle8_full_row_without_eol", R.rle_file(8, 3, [("run", 8, 9), ("run", 8, 10)] + tail, False, pal256)))
    bad.append(("rle4_delta_above_the_image", R.rle_file(8, 3, [("run", 3, 0x12), ("delta", 1, 3)] + tail, True, pal16)))
    bad.append(("rle8_delta_right_of_the_row", R.rle_file(8, 3, [("run", 3, 9), ("delta", 6, 0)] + tail, False, pal256)))
    ones = [("run", 1, 5)] * 63
    bad.append(("rle8_run_past_row_in_the_second_window", R.rle_file(70, 3, ones + [("run", 7, 8), ("eol",), ("run", 69, 1), ("run", 2, 2)] + tail, False, pal256)))
    return good, bad


def mpo_cases():
    """MPO files as Pillow writes them: a JPEG, an APP2 MPF index in it, then a second JPEG of another size."""
    y, x = np.mgrid[0:48, 0:64]
    a = np.stack([(x * 4 + y) & 255, (x + y * 5) & 255, (x * y) & 255], -1).astype(np.uint8)
    b = np.ascontiguousarray(a[:24, :40, ::-1])
    out = []
    for name, kw in (("mpo_two_frames_444", dict(quality=90, subsampling=0)), ("mpo_two_frames_420", dict(quality=75, subsampling=2)),
                     ("mpo_three_frames_gray", dict(quality=85))):
        frames = [Image.fromarray(a), Image.fromarray(b)] + ([Image.fromarray(a[:8, :8])] if "three" in name else [])
        if "gray" in name:
            frames = [f.convert("L") for f in frames]
        buf = io.BytesIO()
        frames[0].save(buf, format="MPO", save_all=True, append_images=frames[1:], **kw)
        out.append((name, buf.getvalue()))
    return out


def pillow_bgr(d):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1])


def main():
    good, bad = cases()
    out = {"names": np.array([n for n, _ in good]), "bad_names": np.array([n for n, _ in bad])}
    judged = {"direct": 0, "rewrite": 0}
    for n, d in good:
        bgr, _, st = R.decode_stages(d)
        assert st == 0, n
        judge = "rewrite" if R.departs(d) else "direct"
        if judge == "rewrite":
            d2 = R.rewrite(d)
            assert not R.departs(d2), n
            bgr2, _, st2 = R.decode_stages(d2)
            assert st2 == 0 and np.array_equal(bgr2, bgr), n
            want = pillow_bgr(d2)
        else:
            want = pillow_bgr(d)
        assert bgr.shape == want.shape and np.array_equal(bgr, want), n
        out["file_" + n] = np.frombuffer(d, np.uint8)
        out["bgr_" + n] = want
        out["judge_" + n] = np.array(judge)
        judged[judge] += 1
    for n, d in bad:
        _, _, st = R.decode_stages(d)
        assert st != 0, n
        out["badfile_" + n] = np.frombuffer(d, np.uint8)
        out["badstatus_" + n] = np.int32(st)
    mpo = mpo_cases()
    out["mpo_names"] = np.array([n for n, _ in mpo])
    for n, d in mpo:
        im = Image.open(io.BytesIO(d))
        assert im.format == "MPO" and im.n_frames >= 2
        im.seek(1)
        assert im.size != Image.open(io.BytesIO(d)).size
        out["mpofile_" + n] = np.frombuffer(d, np.uint8)
        out["mpobgr_" + n] = pillow_bgr(d)
    path = os.path.join(ROOT, "tests", "golden", "bmp_cases.npz")
    np.savez_compressed(path, **out)
    print("%d good (%s), %d malformed, %d MPO, %d bytes -> %s" % (len(good), judged, len(bad), len(mpo), os.path.getsize(path), path))
    print("malformed status:", {n: hex(int(out["badstatus_" + n])) for n, _ in bad})


if __name__ == "__main__":
    main()
