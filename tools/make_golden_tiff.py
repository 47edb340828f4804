"""Writes tests/golden/tiff_cases.npz: the TIFF fixtures of tests/test_tiff_host.py and tests/test_gpu_tiff.py.

    python tools/make_golden_tiff.py

Every good case is a file assembled by hand (tests/tiff_ref.py; Pillow cannot write 4-bit, WhiteIsZero or big-endian files) or written by Pillow,
stored as file_<name> beside bgr_<name>: PILLOW's decode of that file (libtiff), reversed to BGR.  The tool asserts that the rule book
(tiff_ref.decode_stages) gives the same pixels with status 0 before it stores anything, so a fixture is a file on which Pillow and the rule
book agree.  The malformed files are stored as badfile_<name> with badstatus_<name>, the status word the rule book predicts; they are never
compared with Pillow.  Small: every case is at most 64 x 64.
"""
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import tiff_ref as R  # noqa: E402


def cases():
    """-> ([(name, file bytes)], [(name, file bytes)]): the good and the malformed files."""
    rng = np.random.default_rng(7)
    good, bad = [], []
    noise = rng.integers(0, 256, (40, 180), dtype=np.uint8)               # 40 x 60 RGB: 7200 bytes fill the LZW table, walk every width, Clear mid-strip
    y, x = np.mgrid[0:40, 0:60]
    smooth = np.stack([(x * 4 + y) & 255, (x + y * 5) & 255, (x * y) & 255], -1).astype(np.uint8).reshape(40, 180)
    gray = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    # LZW
    good.append(("lzw_rgb_noise_60x40_one_strip", R.assemble(noise, 60, 8, 3, 2, R.LZW)))
    good.append(("lzw_rgb_noise_be_pred2_rps7", R.assemble(noise, 60, 8, 3, 2, R.LZW, predictor=2, rows_per_strip=7, byte_order=">")))
    good.append(("lzw_rgb_smooth_pred2", R.assemble(smooth, 60, 8, 3, 2, R.LZW, predictor=2, rows_per_strip=16)))
    good.append(("lzw_gray_constant_50x3", R.assemble(np.full((3, 50), 77, np.uint8), 50, 8, 1, 1, R.LZW)))
    good.append(("lzw_gray_no_eoi", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(eoi=False))))
    good.append(("lzw_gray_trailing_bytes", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(tail=b"\xff\x00\xaa\x55"))))
    # the device fetches codes 1 .. 64 behind the leading Clear, then 65 .. 128: a Clear on the first and on the last code of a fetch
    good.append(("lzw_gray_clear_first_of_fetch", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(clear_at=(65,)))))
    good.append(("lzw_gray_clear_last_of_fetch", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(clear_at=(64,)))))
    good.append(("lzw_gray_clears_64_129_193", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(clear_at=(64, 129, 193)))))
    good.append(("lzw_gray_double_clear", R.assemble(gray, 16, 8, 1, 1, R.LZW, lzw=dict(clear_at=(1, 2, 30)))))
    good.append(("lzw_gray_1x1", R.assemble(np.array([[200]], np.uint8), 1, 8, 1, 1, R.LZW)))
    good.append(("lzw_gray_pred2_w1", R.assemble(gray[:, :1], 1, 8, 1, 1, R.LZW, predictor=2)))
    rep = np.tile(np.arange(7, dtype=np.uint8) * 31, 64)[:64 * 6].reshape(6, 64)                # long matches: entries made a few codes ago are named at once
    good.append(("lzw_gray_periodic_64x6", R.assemble(rep, 64, 8, 1, 1, R.LZW, rows_per_strip=4)))
    # few symbols: long entries, many of them named within 64 codes of being made (the in-fetch links and the whole-wave copies)
    r2 = np.random.default_rng(9)
    good.append(("lzw_gray_three_values_64x64", R.assemble(r2.integers(0, 3, (64, 64)).astype(np.uint8) * 100, 64, 8, 1, 1, R.LZW, rows_per_strip=40)))
    blocks = np.repeat(r2.integers(0, 256, 80, dtype=np.uint8), r2.integers(1, 100, 80))[:64 * 48].reshape(48, 64)
    good.append(("lzw_gray_runs_64x48_pred2", R.assemble(blocks, 64, 8, 1, 1, R.LZW, predictor=2)))
    # PackBits
    good.append(("packbits_run_128", R.assemble(np.full((2, 64), 9, np.uint8), 64, 8, 1, 1, R.PACKBITS, streams={0: bytes([0x81, 9])})))
    lit = rng.integers(0, 256, (2, 64), dtype=np.uint8)
    good.append(("packbits_literal_128", R.assemble(lit, 64, 8, 1, 1, R.PACKBITS, streams={0: bytes([127]) + lit.tobytes()})))
    g8 = gray[:1, :8]
    good.append(("packbits_nop_headers", R.assemble(g8, 8, 8, 1, 1, R.PACKBITS, streams={0: bytes([0x80, 3]) + g8.tobytes()[:4] + bytes([0x80, 0x80, 3]) + g8.tobytes()[4:]})))
    runs = np.repeat(np.array([5, 5, 5, 200, 200, 17], np.uint8), 10).reshape(6, 10)[:4]
    runs[1:3] = 5                                                                             # one run across two row ends
    good.append(("packbits_run_crosses_rows", R.assemble(runs, 10, 8, 1, 1, R.PACKBITS)))
    good.append(("packbits_rgb_noise_rps3", R.assemble(noise[:10, :33], 11, 8, 3, 2, R.PACKBITS, rows_per_strip=3)))
    # Deflate
    good.append(("deflate_stored", R.assemble(gray, 16, 8, 1, 1, R.ADOBE_DEFLATE, level=0)))
    fixed = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    good.append(("deflate_fixed", R.assemble(smooth[:8, :48], 16, 8, 3, 2, R.ADOBE_DEFLATE, streams={0: fixed.compress(smooth[:8, :48].tobytes()) + fixed.flush()})))
    skew = np.random.default_rng(8).choice(np.array([0, 0, 0, 0, 0, 1, 1, 2, 3, 50, 200, 255], np.uint8), (40, 180))      # a skewed alphabet: a dynamic block
    good.append(("deflate_dynamic_32946", R.assemble(skew, 60, 8, 3, 2, R.DEFLATE, level=9)))
    good.append(("deflate_pred2_three_strips", R.assemble(smooth, 60, 8, 3, 2, R.ADOBE_DEFLATE, predictor=2, rows_per_strip=14)))
    good.append(("deflate_gray_pred2_be", R.assemble(smooth[:, :60], 60, 8, 1, 1, R.ADOBE_DEFLATE, predictor=2, byte_order=">", rows_per_strip=13)))
    # pixels
    b1 = rng.integers(0, 2, (9, 13))
    b4 = rng.integers(0, 16, (7, 5))
    for ph, word in ((0, "white_is_zero"), (1, "black_is_zero")):
        good.append(("bilevel_13x9_" + word, R.assemble(R.pack(b1, 1), 13, 1, 1, ph, rows_per_strip=4)))
        good.append(("gray4_5x7_" + word, R.assemble(R.pack(b4, 4), 5, 4, 1, ph, R.LZW, byte_order=">" if ph else "<")))
        good.append(("gray8_16x16_" + word, R.assemble(gray, 16, 8, 1, ph, R.PACKBITS)))
    cm4 = rng.integers(0, 65536, 48)
    cm8 = rng.integers(0, 65536, 768)
    good.append(("palette4_5x7", R.assemble(R.pack(b4, 4), 5, 4, 1, 3, R.ADOBE_DEFLATE, colormap=cm4)))
    good.append(("palette8_16x16_be", R.assemble(gray, 16, 8, 1, 3, R.LZW, colormap=cm8, byte_order=">")))
    good.append(("gray8_w1", R.assemble(gray[:, :1], 1, 8, 1, 1)))
    good.append(("rgb8_w1", R.assemble(gray[:, :3], 1, 8, 3, 2)))
    good.append(("rgb8_one_strip_short_offsets", R.assemble(noise[:5, :21], 7, 8, 3, 2, strip_type=R.SHORT)))
    good.append(("rgb8_many_strips_long_offsets", R.assemble(noise[:9, :21], 7, 8, 3, 2, rows_per_strip=1, size_type=R.LONG)))
    good.append(("rgb8_rows_per_strip_above_h", R.assemble(noise[:5, :21], 7, 8, 3, 2, R.LZW, rows_per_strip=100000)))
    # what Pillow writes
    for comp in ("tiff_lzw", "tiff_adobe_deflate", "packbits", "raw"):
        buf = io.BytesIO()
        Image.fromarray(smooth.reshape(40, 60, 3)).save(buf, "TIFF", compression=comp)
        good.append(("pillow_" + comp, buf.getvalue()))
    # malformed: status bits, never Pillow
    bad.append(("lzw_code_above_next_free", R.assemble(np.zeros((1, 16), np.uint8), 16, 8, 1, 1, R.LZW,
                                                       streams={0: R.pack_codes([(256, 9), (65, 9), (66, 9), (300, 9), (257, 9)])})))
    z = R.lzw_encode(gray.tobytes())
    bad.append(("lzw_truncated", R.assemble(gray, 16, 8, 1, 1, R.LZW, streams={0: z[:len(z) // 2]})))
    bad.append(("packbits_literal_off_the_strip", R.assemble(np.zeros((1, 16), np.uint8), 16, 8, 1, 1, R.PACKBITS, streams={0: bytes([10, 1, 2, 3])})))
    bad.append(("deflate_block_type_3", R.assemble(np.zeros((2, 16), np.uint8), 16, 8, 1, 1, R.ADOBE_DEFLATE, streams={0: b"\x78\x9c\x07" + bytes(8)})))
    zz = zlib.compress(gray.tobytes(), 9)
    bad.append(("deflate_truncated", R.assemble(gray, 16, 8, 1, 1, R.ADOBE_DEFLATE, streams={0: zz[:len(zz) // 2]})))
    return good, bad


def main():
    assert features.check("libtiff"), "Pillow without libtiff: no judge"
    good, bad = cases()
    out = {"names": np.array([n for n, _ in good]), "bad_names": np.array([n for n, _ in bad])}
    for n, d in good:
        want = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1])
        bgr, _, st = R.decode_stages(d)
        assert st == 0 and bgr.shape == want.shape and np.array_equal(bgr, want), n
        assert max(want.shape[:2]) <= 64, n
        out["file_" + n] = np.frombuffer(d, np.uint8)
        out["bgr_" + n] = want
    for n, d in bad:
        _, _, st = R.decode_stages(d)
        assert st != 0, n
        out["badfile_" + n] = np.frombuffer(d, np.uint8)
        out["badstatus_" + n] = np.int32(st)
    path = os.path.join(ROOT, "tests", "golden", "tiff_cases.npz")
    np.savez_compressed(path, **out)
    print("%d good, %d malformed, %d bytes -> %s" % (len(good), len(bad), os.path.getsize(path), path))
    print("malformed status:", {n: hex(int(out["badstatus_" + n])) for n, _ in bad})


if __name__ == "__main__":
    main()
