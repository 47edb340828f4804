"""No GPU: the JPEG marker walk (maf-yolo_amd/jpeg.py parse) and the NumPy restatement of libjpeg's baseline decoder (tests/jpeg_ref.py).

* jpeg_ref.decode equals the fixture pixels (tests/golden/jpeg_cases.npz, written by tools/make_golden_jpeg.py with Pillow / libjpeg-turbo)
  exactly for every case, the 480 x 640 one by its sha256; where Pillow is importable it also equals a fresh Pillow decode;
* parse reads size, components, sampling, restart interval and table counts of every case;
* every unsupported kind raises JpegUnsupported naming it (a progressive and an EXIF orientation 6 file from Pillow, the others by editing
  header bytes); truncated header segments, a missing table and a missing EOI raise a plain MafError.
"""
import hashlib
import io

import numpy as np
import pytest

import jpeg_ref as R
from maf_yolo_amd import jpeg as J
from maf_yolo_amd.lib import MafError


@pytest.fixture(scope="module")
def cases(golden):
    return golden("jpeg_cases")


def _names(z):
    return [str(n) for n in z["names"]]


def _segments(d):
    """[(marker, offset of the 0xFF, segment length field)] of the header up to and including SOS."""
    out, p = [], 2
    while True:
        assert d[p] == 0xFF
        m, L = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        out.append((m, p, L))
        if m == 0xDA:
            return out
        p += 2 + L


def _seg(d, marker):
    return next((p, L) for m, p, L in _segments(d) if m == marker)


def _edit(d, at, value):
    b = bytearray(d)
    b[at] = value
    return bytes(b)


def test_restatement_equals_the_fixture_pixels(cases):
    for n in _names(cases):
        got = R.decode(cases["file_" + n].tobytes())
        want = cases["bgr_" + n]
        assert got.dtype == np.uint8 and got.shape == want.shape, n
        assert np.array_equal(got, want), n


def test_restatement_large_case_sha256(cases):
    got = R.decode(cases["large_file"].tobytes())
    assert got.shape == (480, 640, 3)
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(cases["large_sha256"])


def test_restatement_equals_a_fresh_pillow_decode(cases):
    Image = pytest.importorskip("PIL.Image")
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]
        assert np.array_equal(R.decode(d), want), n
        assert np.array_equal(cases["bgr_" + n], want), n


def test_parse_reads_every_case(cases):
    rst_markers = {}
    for n, meta in zip(_names(cases), cases["meta"].tolist()):
        h, w, nc, hs, vs, ri, nq, nh, _ = meta
        d = cases["file_" + n].tobytes()
        info = J.parse(d)
        assert (info.height, info.width, len(info.components), info.precision) == (h, w, nc, 8), n
        assert (info.components[0].h, info.components[0].v) == (hs, vs), n
        assert all((c.h, c.v) == (1, 1) for c in info.components[1:]), n
        assert info.restart_interval == ri, n
        assert len(info.qtables) == nq and len(info.huffman) == nh, n
        assert all(t.shape == (64,) and t.dtype == np.uint16 for t in info.qtables.values())
        assert info.orientation is None
        s, e = info.scan
        assert d[s - 13 if nc == 3 else s - 9] == 0xDA and d[e:e + 2] == b"\xff\xd9" and e + 2 == len(d), n
        a = np.frombuffer(d[s:e], np.uint8)
        rst_markers[n] = int(((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)).sum())
        mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
        assert rst_markers[n] == (-(-mcus // ri) - 1 if ri else 0), n
    assert rst_markers["grad_q75_rst2_17x33_s0"] == 7                 # wraps the modulo-8 RSTn index
    q = J.parse(cases["file_grad_q75_8x8_s0"].tobytes()).qtables[0]
    annex_k = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                        72, 92, 95, 98, 112, 100, 103, 99])       # the luminance table of JPEG Annex K, row-major
    assert np.array_equal(q, np.maximum((annex_k * 50 + 50) // 100, 1))     # de-zigzagged; quality 75 scales by 50 % (jcparam.c)


def test_optimised_huffman_tables_differ_from_the_standard_ones(cases):
    std = J.parse(cases["file_grad_q75_17x33_s2"].tobytes()).huffman
    opt = J.parse(cases["file_noise_q30_opt_17x33_s2"].tobytes()).huffman
    assert any(not np.array_equal(std[k][0], opt[k][0]) for k in std)


def test_unsupported_kinds_are_named(cases):
    base = cases["file_grad_q75_17x33_s2"].tobytes()
    sof, _ = _seg(base, 0xC0)
    dqt, _ = _seg(base, 0xDB)
    sos, _ = _seg(base, 0xDA)

    def raises(d, word):
        with pytest.raises(J.JpegUnsupported, match=word):
            J.parse(d)
        assert not J.supported(d)

    raises(cases["progressive_file"].tobytes(), "progressive")
    raises(_edit(base, sof + 1, 0xC2), "progressive")
    raises(_edit(base, sof + 1, 0xC1), "SOF1")
    raises(_edit(base, sof + 1, 0xC9), "arithmetic")
    raises(_edit(base, sof + 4, 12), "12-bit")
    raises(_edit(base, dqt + 4, 0x10), "16-bit quantisation")
    raises(_edit(base, sof + 9, 4), "4 components")
    raises(_edit(base, sos + 4, 1), "more than one scan")
    raises(base[:-2] + base[sos:sos + 14] + b"\x00\xff\xd9", "more than one scan")
    raises(_edit(base, sof + 11, 0x12), "sampling")
    raises(_edit(base, sof + 11, 0x41), "sampling")
    raises(_edit(base, sof + 14, 0x22), "sampling")
    assert J.supported(base)
    # EXIF orientation: parse reports it, supported() says no (cv2.imread would rotate)
    o6 = cases["orientation6_file"].tobytes()
    assert J.parse(o6).orientation == 6 and not J.supported(o6)


def test_malformed_files_raise_maferror(cases):
    base = cases["file_grad_q75_17x33_s2"].tobytes()
    segs = _segments(base)

    def raises(d, word):
        with pytest.raises(MafError, match=word) as e:
            J.parse(d)
        assert not isinstance(e.value, J.JpegUnsupported)
        assert not J.supported(d)

    raises(b"", "SOI")
    raises(base[1:], "SOI")
    raises(base[:-2], "EOI")                                         # the scan runs to the end of the file
    for m, p, L in segs:                                             # every header segment cut in the middle
        raises(base[:p + 2 + L // 2], "past the end|cut short|no SOS")
    dqt, L = _seg(base, 0xDB)
    raises(base[:dqt] + base[dqt + 2 + L:], "quantisation table . is missing")
    dht, L = _seg(base, 0xC4)
    raises(base[:dht] + base[dht + 2 + L:], "Huffman table")
    info = J.parse(base)
    half = base[:info.scan[0] + (info.scan[1] - info.scan[0]) // 2] + b"\xff\xd9"
    assert J.supported(half)                                         # the header is intact: only the decoder can tell
    coefs, status = R.coefficients(half)
    assert status & J.STATUS_SHORT_SCAN


def test_device_huffman_table_agrees_with_the_canonical_codes(cases):
    for n in ("grad_q75_17x33_s2", "noise_q30_opt_75x100_s2", "noise_q100_75x100_s0"):
        for (tc, th), (bits, vals) in J.parse(cases["file_" + n].tobytes()).huffman.items():
            t = J.huff_device_table(bits, vals)
            look, maxcode, valoff, huffval = t[:1024].view("<u2"), t[1024:1096].view("<i4"), t[1096:1168].view("<i4"), t[1168:]
            mincode, mx, valptr, v = R._canon(bits, vals)
            for l in range(1, 17):
                for code in range(mincode[l], mx[l] + 1):
                    sym = v[valptr[l] + code - mincode[l]]
                    if l <= J.HUFF_LOOK_BITS:
                        lo = code << (9 - l)
                        assert (look[lo:lo + (1 << (9 - l))] == ((l << 8) | sym)).all()
                    else:
                        assert look[code >> (l - 9)] == 0 and maxcode[l] == mx[l] and huffval[valoff[l] + code] == sym
