"""Writes tests/golden/jpeg_progressive_cases.npz with Pillow (libjpeg-turbo): the synthetic images of tools/make_golden_jpeg.py encoded as
PROGRESSIVE JPEG files (progressive=True: libjpeg's jpeg_simple_progression, 10 scans for YCbCr, 6 for gray, optimised Huffman tables per
scan) and the pixels Pillow decodes from them with libjpeg's defaults, stored BGR — what cv2.imread returns for the same bytes.

    python tools/make_golden_jpeg_progressive.py

Keys as in jpeg_cases.npz: names [n]; file_<name> uint8 (the JPEG bytes); bgr_<name> uint8 [h, w, 3] (expected frame); meta int32 [n, 9] = h,
w, components, Y sampling h, v, restart interval (in MCUs of each scan: blocks in the one-component scans; for the restart_marker_rows cases that of the interleaved scans,
libjpeg sets one MCU row of EACH scan's own grid there), quantisation tables, scans,
1 (a progressive file's Huffman tables are always optimised) — known from how each file was written, not read back with the parser under test;
large_file / large_sha256 (480 x 640, 4:2:0, q 90: the sha256 of the expected BGR bytes).  One case, grad_q75_rst2_longeob_17x33_s0, is a
Pillow file with one bit set afterwards (long_eob_run below).  Pillow writes no other scan script than
jpeg_simple_progression; scripts beyond it are not covered.

After writing, the script decodes every case with tests/jpeg_progressive_ref.py and prints its branch counters: each must be above zero
(tests/test_jpeg_progressive_host.py asserts it), so a change of the cases that loses a branch shows here first.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from make_golden_jpeg import SAMPLING, SIZES, encode, expected, gradient, noise, smooth_texture  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_progressive_cases.npz")


def long_eob_run(data):
    """libjpeg's encoder ends every EOB run at a restart marker (jcphuff.c emit_restart flushes it), so in the files Pillow writes the decoder's
    EOBRUN is already 0 when process_restart of jdphuff.c resets it.  This makes the one case where it is not, without an encoder: in an AC
    first pass it finds an EOBr symbol whose run ends exactly with its restart interval and sets the low extra bit of the run length (a bit that
    is 0, in a byte that neither is nor becomes 0xFF), so the run claims one block more than the interval has.  A decoder that resets EOBRUN
    at the restart decodes the same pixels as before (Pillow does: asserted here); one that carries it over skips a block."""
    import jpeg_progressive_ref as P
    from maf_yolo_amd import jpeg as J
    info = J.parse(data, progressive=True)
    P.TRACE = []
    P.coefficients(data, info)
    trace, P.TRACE = P.TRACE, None
    for si, k, bit, r, m, run in trace:
        sc = info.scans[si]
        gw, gh = J.scan_geometry(info, sc)
        ri = sc.restart_interval
        if not ri or (k + 1) * ri >= gw * gh or m + run != (k + 1) * ri or run & 1:
            continue
        b0, b1 = J._restart_ranges(data, sc.range, -(-gw * gh // ri))[k]
        at = b0 + ((bit + r - 1) >> 3)
        mask = 0x80 >> ((bit + r - 1) & 7)
        if 0xFF in data[b0:b1] or data[at] & mask or (data[at] | mask) == 0xFF:
            continue
        out = bytearray(data)
        out[at] |= mask
        out = bytes(out)
        assert np.array_equal(expected(out), expected(data))
        return out
    raise SystemExit("no EOB run ends with its restart interval: pick another source case")


def main():
    cases = []          # (name, bytes, meta)

    def add(name, rgb, q, ss, optimize=False, blocks=0, rows=0):
        h, w = rgb.shape[:2]
        kw = {"progressive": True}
        if optimize:
            kw["optimize"] = True
        if blocks:
            kw["restart_marker_blocks"] = blocks
        if rows:
            kw["restart_marker_rows"] = rows
        data = encode(rgb, q, ss, **kw)
        nc = 3 if rgb.ndim == 3 else 1
        hs, vs = SAMPLING[ss] if nc == 3 else (1, 1)
        mcux = -(-w // (8 * hs))
        ri = blocks if blocks else rows * mcux
        cases.append((name, data, [h, w, nc, hs, vs, ri, 2 if nc == 3 else 1, 10 if nc == 3 else 6, 1]))

    for h, w in SIZES:
        for ss in (0, 1, 2):
            add("grad_q75_%dx%d_s%d" % (h, w, ss), gradient(h, w), 75, ss)
            add("noise_q30_opt_%dx%d_s%d" % (h, w, ss), noise(h, w, 10 + h), 30, ss, optimize=True)
    for i, (h, w) in enumerate([(8, 8), (17, 33), (75, 100)]):
        for ss in (0, 1, 2):
            add("noise_q100_%dx%d_s%d" % (h, w, ss), noise(h, w, 20 + i), 100, ss)
    for ss in (0, 1, 2):
        add("grad_q75_rst2_17x33_s%d" % ss, gradient(17, 33), 75, ss, blocks=2)
    add("noise_q30_opt_rst2_75x100_s2", noise(75, 100, 30), 30, 2, optimize=True, blocks=2)
    for ss in (0, 1, 2):
        add("grad_q75_rstrow_48x64_s%d" % ss, gradient(48, 64), 75, ss, rows=1)
    add("gray_q75_17x33", gradient(17, 33)[..., 0] // 2 + gradient(17, 33)[..., 2] // 2, 75, 0)

    cases.append(("grad_q75_rst2_longeob_17x33_s0", long_eob_run(cases[[c[0] for c in cases].index("grad_q75_rst2_17x33_s0")][1]),
                  [17, 33, 3, 1, 1, 2, 2, 10, 1]))

    out = {"names": np.array([c[0] for c in cases]), "meta": np.array([c[2] for c in cases], np.int32)}
    for name, data, _ in cases:
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["bgr_" + name] = expected(data)
    large = encode(smooth_texture(480, 640, 40), 90, 2, progressive=True)
    out["large_file"] = np.frombuffer(large, np.uint8)
    out["large_sha256"] = np.array(hashlib.sha256(expected(large).tobytes()).hexdigest())
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))

    import jpeg_progressive_ref as P
    P.reset_counters()
    for name, data, _ in cases:
        assert np.array_equal(P.decode(data), out["bgr_" + name]), name
    print("branch counters over the cases:", P.COUNTERS)
    assert all(P.COUNTERS.values()), "a branch of jdphuff.c is not reached: add a case"


if __name__ == "__main__":
    main()
