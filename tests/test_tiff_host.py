"""No GPU: the IFD walk (maf-yolo_amd/tiff.py parse), the rule book and the hand assembler (tests/tiff_ref.py), the hand-written binding and
the router.

* tiff_ref equals the fixtures (tests/golden/tiff_cases.npz, written by tools/make_golden_tiff.py: Pillow's pixels) and, where Pillow has libtiff,
  a fresh Pillow decode of every fixture and of files assembled here; it predicts the stored status word of every malformed fixture;
* the LZW and PackBits encoders round-trip, and the closed form for the width of the k-th code behind a Clear (what the device fetches by) equals
  the widths the serial decoder walks through;
* parse reads every case; each unsupported kind is named in its TiffUnsupported; corrupt IFDs raise MafError; decode names the offending file
  before the device is touched;
* blob layout and alignment; the struct sizes equal maf_tiff_struct_sizes of the built library;
* the prototypes of include/mafyolo_tiff.h, read by regex, equal tiff.py's argtypes and restype; neither function is in lib.EXPORTS or
  mafyolo_hip.h;
* the router: without tiff=True a TIFF file is refused exactly as before, with it order and hand-on of the flags are right (fakes).
"""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

import tiff_ref as R
from maf_yolo_amd import frames as F, jpeg as J, lib, png as P, tiff as T, webp as W, webp_lossy as WL
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow():
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check("libtiff") else None


needs_pillow = pytest.mark.skipif(_pillow() is None, reason="Pillow without libtiff: the judge of the rule book is absent")


@pytest.fixture(scope="module")
def cases(golden):
    return golden("tiff_cases")


def _names(z, key="names"):
    return [str(n) for n in z[key]]


def _gray(seed=5, h=6, w=9):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _file(**kw):
    g = _gray()
    return R.assemble(g, 9, 8, 1, 1, **kw)


def test_rule_book_equals_the_fixtures(cases):
    names = _names(cases)
    assert len(names) >= 40
    for word in ("lzw_rgb_noise_60x40_one_strip", "lzw_rgb_noise_be_pred2_rps7", "lzw_gray_constant_50x3", "lzw_gray_no_eoi", "lzw_gray_trailing_bytes",
                 "lzw_gray_clear_first_of_fetch", "lzw_gray_clear_last_of_fetch", "lzw_gray_1x1", "packbits_run_128", "packbits_literal_128",
                 "packbits_nop_headers", "packbits_run_crosses_rows", "packbits_rgb_noise_rps3", "deflate_stored", "deflate_fixed", "deflate_dynamic_32946",
                 "deflate_pred2_three_strips", "bilevel_13x9_white_is_zero", "bilevel_13x9_black_is_zero", "gray4_5x7_white_is_zero",
                 "gray4_5x7_black_is_zero", "palette4_5x7", "palette8_16x16_be", "gray8_w1", "rgb8_w1", "rgb8_one_strip_short_offsets",
                 "rgb8_many_strips_long_offsets", "rgb8_rows_per_strip_above_h"):
        assert word in names, word
    for n in names:
        d = cases["file_" + n].tobytes()
        bgr, _, st = R.decode_stages(d)
        assert st == 0 and bgr.dtype == np.uint8 and np.array_equal(bgr, cases["bgr_" + n]), n
        assert max(bgr.shape[:2]) <= 64, n


def test_the_cases_reach_their_edges(cases):
    """The fixtures are what their names say: the table fills, every width is walked, the deflate block types occur, the offsets are inline."""
    d = cases["file_lzw_rgb_noise_60x40_one_strip"].tobytes()
    _, t = R.read_ifd(d)
    assert len(t[273]) == 1
    strip = d[t[273][0]:t[273][0] + t[279][0]]
    # walk the codes with the serial decoder's widths
    widths, clears = _walk_widths(strip, 7200)
    assert set(widths) == {9, 10, 11, 12} and clears >= 2
    _, t = R.read_ifd(cases["file_lzw_rgb_noise_be_pred2_rps7"].tobytes())
    assert len(t[273]) == 6 and t[278] == [7] and t[317] == [2]
    _, t = R.read_ifd(cases["file_rgb8_one_strip_short_offsets"].tobytes())
    assert len(t[273]) == 1
    _, t = R.read_ifd(cases["file_rgb8_rows_per_strip_above_h"].tobytes())
    assert t[278][0] > t[257][0]
    import png_ref
    for n, key in (("deflate_stored", "stored"), ("deflate_fixed", "fixed"), ("deflate_dynamic_32946", "dynamic")):
        d = cases["file_" + n].tobytes()
        _, t = R.read_ifd(d)
        c = png_ref.new_counters()
        png_ref.inflate(d[t[273][0]:t[273][0] + t[279][0]], t[257][0] * ((t[256][0] * len(t[258]) * 8 + 7) // 8), c)
        assert c[key] >= 1, n
    assert R.read_ifd(cases["file_deflate_dynamic_32946"].tobytes())[1][259] == [32946]
    assert len(R.read_ifd(cases["file_deflate_pred2_three_strips"].tobytes())[1][273]) == 3


def _walk_widths(strip, total):
    """The widths of the codes of an LZW strip, by the serial rule (next free entry against 2^width - 2), and the number of Clears."""
    nbits = len(strip) * 8
    acc = int.from_bytes(strip, "big")
    pos, width, free, out, widths, clears, first = 0, 9, 258, 0, [], 0, True
    lens = {}
    prev = 0
    while out < total and pos + width <= nbits:
        code = (acc >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        widths.append(width)
        if code == 256:
            width, free, first, lens = 9, 258, True, {}
            clears += 1
            continue
        if code == 257:
            break
        n = 1 if code < 256 else lens[code] if code < free else prev + 1
        if not first:
            lens[free] = prev + 1
            free += 1
            if free > (1 << width) - 2 and width < 12:
                width += 1
        first = False
        prev = n
        out += n
    return widths, clears


def test_the_width_of_a_code_depends_on_its_index_alone():
    """What the device fetches by: the k-th code behind a Clear has lzw_width(k) bits, whatever the data."""
    rng = np.random.default_rng(2)
    for data in (rng.integers(0, 256, 6000, dtype=np.uint8), rng.integers(0, 4, 30000).astype(np.uint8), np.zeros(9000, np.uint8)):
        strip = R.lzw_encode(data.tobytes(), clear_at=(700,))
        widths, clears = _walk_widths(strip, len(data))
        k = 0
        for (code, wd), serial in zip(R.lzw_codes(data.tobytes(), clear_at=(700,)), widths):
            assert wd == serial == R.lzw_width(k)
            k = 0 if code == 256 else k + 1
        got, st = R.lzw_decode(strip, len(data))
        assert st == 0 and np.array_equal(got, data)
    assert [R.lzw_width(m) for m in (0, 253, 254, 765, 766, 1789, 1790, 4000)] == [9, 9, 10, 10, 11, 11, 12, 12]


def test_encoders_round_trip():
    rng = np.random.default_rng(4)
    for data in (rng.integers(0, 256, 500, dtype=np.uint8), np.repeat(rng.integers(0, 256, 40, dtype=np.uint8), rng.integers(1, 300, 40)), np.zeros(1, np.uint8)):
        got, st = R.packbits_decode(R.packbits_encode(data.tobytes()), len(data))
        assert st == 0 and np.array_equal(got, data)
        for kw in (dict(), dict(eoi=False), dict(tail=b"\x01\x02"), dict(clear_at=(1, 64, 65))):
            got, st = R.lzw_decode(R.lzw_encode(data.tobytes(), **kw), len(data))
            assert st == 0 and np.array_equal(got, data), kw
    # a table that is never cleared overflows: the status, not a crash
    data = rng.integers(0, 256, 9000, dtype=np.uint8)
    got, st = R.lzw_decode(R.lzw_encode(data.tobytes(), limit=10 ** 9), 9000)
    assert st == R.ST_LZW_TABLE_FULL and not got[-100:].any()


@needs_pillow
def test_fixtures_equal_a_fresh_pillow_decode(cases):
    Image = _pillow()
    for n in _names(cases):
        want = np.asarray(Image.open(io.BytesIO(cases["file_" + n].tobytes())).convert("RGB"))[..., ::-1]
        assert np.array_equal(cases["bgr_" + n], want), n


@needs_pillow
def test_rule_book_equals_pillow_on_fresh_files():
    Image = _pillow()
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:23, 0:31]
    rgb = np.stack([(x * 7 + y) & 255, (x + y * 3) & 255, (x * y) & 255], -1).astype(np.uint8)
    rgb[5:12, 3:20] = rng.integers(0, 256, (7, 17, 3), dtype=np.uint8)
    n = 0
    for comp in (R.NONE, R.LZW, R.ADOBE_DEFLATE, R.DEFLATE, R.PACKBITS):
        for bo in "<>":
            for rps in (None, 1, 5, 23, 4000):
                for pred in (1, 2) if comp in (R.LZW, R.ADOBE_DEFLATE, R.DEFLATE) else (1,):
                    for spp in (1, 3):
                        rows = rgb.reshape(23, 93) if spp == 3 else rgb[:, :, 0]
                        d = R.assemble(rows, 31, 8, spp, 2 if spp == 3 else n % 2, comp, predictor=pred, rows_per_strip=rps, byte_order=bo,
                                       strip_type=R.SHORT if n % 3 == 0 else R.LONG, size_type=R.LONG if n % 2 else R.SHORT)
                        want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]
                        bgr, _, st = R.decode_stages(d)
                        assert st == 0 and np.array_equal(bgr, want), (comp, bo, rps, pred, spp)
                        info = T.parse(d)
                        assert (info.height, info.width) == bgr.shape[:2] and info.byte_order == bo and T.supported(d)
                        n += 1
    for bits, w in ((1, 13), (1, 8), (4, 5), (4, 6)):
        s = rng.integers(0, 1 << bits, (7, w))
        for ph in (0, 1) + ((3,) if bits == 4 else ()):
            d = R.assemble(R.pack(s, bits), w, bits, 1, ph, R.LZW, rows_per_strip=3, colormap=rng.integers(256, 65536, 48) if ph == 3 else None)
            want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]
            assert np.array_equal(R.decode(d), want) and T.supported(d), (bits, w, ph)
    for comp in ("tiff_lzw", "tiff_adobe_deflate", "tiff_deflate", "packbits", "raw"):
        for mode in ("RGB", "L", "P", "1"):
            buf = io.BytesIO()
            Image.fromarray(rgb).convert(mode).save(buf, "TIFF", compression=comp)
            d = buf.getvalue()
            want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]
            assert np.array_equal(R.decode(d), want) and T.supported(d), (comp, mode)


def test_rule_book_predicts_the_malformed_status(cases):
    want = {"lzw_code_above_next_free": T.STATUS_LZW_BAD_CODE, "lzw_truncated": T.STATUS_INPUT_EXHAUSTED, "packbits_literal_off_the_strip": T.STATUS_PACKBITS_OVERRUN,
            "deflate_block_type_3": 2 << T.STATUS_INFLATE_SHIFT, "deflate_truncated": 1 << T.STATUS_INFLATE_SHIFT}
    assert sorted(_names(cases, "bad_names")) == sorted(want)
    for n, w in want.items():
        d = cases["badfile_" + n].tobytes()
        assert T.supported(d), n                                      # the IFD is intact: only the decoder can tell
        _, _, st = R.decode_stages(d)
        assert st == int(cases["badstatus_" + n]) == w, n
    assert (T.STATUS_INPUT_EXHAUSTED, T.STATUS_LZW_BAD_CODE, T.STATUS_LZW_TABLE_FULL, T.STATUS_PACKBITS_OVERRUN, T.STATUS_INFLATE_SHIFT) == (
        R.ST_INPUT_EXHAUSTED, R.ST_LZW_BAD_CODE, R.ST_LZW_TABLE_FULL, R.ST_PACKBITS_OVERRUN, R.ST_INFLATE_SHIFT) == (1, 2, 4, 8, 8)
    assert T.status_text(3) == "a strip that ends before its rows are full, an LZW code above the next free entry"
    assert T.status_text(0x200) == "a corrupt Deflate strip"


def test_parse_reads_every_case(cases):
    for n in _names(cases) + _names(cases, "bad_names"):
        d = cases[("file_" if "file_" + n in cases else "badfile_") + n].tobytes()
        bo, t = R.read_ifd(d)
        info = T.parse(d)
        h = t[257][0]
        rps = min(t.get(278, [h])[0], h)
        assert (info.width, info.height, info.bits, info.spp, info.photometric) == (t[256][0], h, t.get(258, [1])[0], t.get(277, [1])[0], t[262][0]), n
        assert (info.compression, info.predictor, info.rows_per_strip, info.byte_order) == (t.get(259, [1])[0], t.get(317, [1])[0], rps, bo), n
        assert info.strips == tuple((o, o + c) for o, c in zip(t[273], t[279]))[:-(-h // rps)] and len(info.strips) == -(-h // rps), n
        assert info.row_bytes == (info.width * info.spp * info.bits + 7) // 8 and info.orientation == 1, n
        if info.photometric == 3:
            assert np.array_equal(info.palette, (np.array(t[320]).reshape(3, -1).T >> 8).astype(np.uint8)), n
        else:
            assert info.palette is None, n


def test_unsupported_kinds_are_named():
    g = _gray()
    rgb = np.random.default_rng(6).integers(0, 256, (6, 27), dtype=np.uint8)

    def raises(d, word, **kw):
        with pytest.raises(T.TiffUnsupported, match=word):
            T.parse(d, **kw)
        assert not T.supported(d, **kw)

    assert T.supported(_file())
    raises(R.assemble(g, 9, 8, 1, 1, magic=43), "BigTIFF")
    raises(_file(extra={322: (R.SHORT, [16]), 323: (R.SHORT, [16])}), "tiles")
    raises(_file(extra={324: (R.LONG, [8])}), "tiles")
    raises(R.assemble(rgb, 9, 8, 3, 2, extra={284: (R.SHORT, [2])}), "PlanarConfiguration 2")
    assert T.supported(_file(extra={284: (R.SHORT, [2])}))               # one sample per pixel: the two layouts are the same
    raises(R.assemble(np.zeros((6, 18), np.uint8), 9, 16, 1, 1), "16-bit samples")
    raises(R.assemble(np.zeros((6, 36), np.uint8), 9, 32, 1, 1), "32-bit samples")
    raises(R.assemble(np.zeros((6, 36), np.uint8), 9, 32, 1, 1, extra={339: (R.SHORT, [3])}), "sample format 3 .*float")
    raises(R.assemble(np.zeros((6, 3), np.uint8), 9, 2, 1, 1), "2-bit samples")
    raises(R.assemble(np.zeros((6, 36), np.uint8), 9, 8, 4, 2, extra={338: (R.SHORT, [2])}), "ExtraSamples")
    raises(R.assemble(np.zeros((6, 36), np.uint8), 9, 8, 4, 2), "4 samples per pixel")
    raises(R.assemble(np.zeros((6, 18), np.uint8), 9, 8, 2, 1), "2 samples per pixel")
    raises(R.assemble(rgb, 9, 8, 3, 6), "photometric interpretation 6")
    raises(R.assemble(rgb, 9, 8, 3, 1), "photometric interpretation 1 with 3 samples")
    raises(_file(extra={256: (R.LONG, [70000])}), "70000 x 6 is beyond")
    raises(R.assemble(rgb, 9, 8, 3, 2, extra={256: (R.LONG, [65535]), 257: (R.LONG, [20000])}), "beyond the 2 GiB of rows")
    raises(_file(extra={259: (R.SHORT, [7])}), "compression 7")
    raises(_file(extra={259: (R.SHORT, [4])}), "compression 4")
    raises(_file(extra={266: (R.SHORT, [2])}), "FillOrder 2")
    for o in (2, 6, 8):
        d = _file(extra={274: (R.SHORT, [o])})
        raises(d, "Orientation of %d" % o)
        assert T.supported(d, ignore_orientation=True) and T.parse(d, ignore_orientation=True).orientation == o
    raises(R.assemble(g, 9, 8, 1, 3, colormap=np.arange(768) % 256), "palette whose entries are all below 256")
    raises(_file(extra={50706: (R.BYTE, [1, 4, 0, 0])}), "DNG")
    raises(_file(compression=R.LZW, streams={0: b"\x00\x01\x02\x03"}), "does not begin with the Clear code 256")
    old_style = bytes([0x00, 0x01]) + bytes(6)                           # LSB-first LZW begins 0x00 0x01
    raises(_file(compression=R.LZW, streams={0: old_style}), "old-style LZW")
    raises(_file(compression=R.PACKBITS, predictor=2), "predictor 2 with compression 32773")
    raises(_file(compression=R.LZW, extra={317: (R.SHORT, [3])}), "predictor 3")
    raises(_file(compression=R.ADOBE_DEFLATE, streams={0: b"\x78\xbb" + bytes(4)}), "preset dictionary")
    with pytest.raises(T.TiffUnsupported, match=r"file 1: tiff: FillOrder 2"):
        T.decode([_file(), _file(extra={266: (R.SHORT, [2])})], device="cuda:0")      # parsed before the device is touched
    assert issubclass(T.TiffUnsupported, MafError)


def test_corrupt_ifds_raise_maferror():
    good = _file(rows_per_strip=2)
    assert T.supported(good)
    bo, t = R.read_ifd(good)
    ifd, = struct.unpack("<I", good[4:8])

    def raises(d, word):
        with pytest.raises(MafError, match=word) as e:
            T.parse(d)
        assert not isinstance(e.value, T.TiffUnsupported) and not T.supported(d)

    def entry(tag):
        n, = struct.unpack("<H", good[ifd:ifd + 2])
        for i in range(n):
            at = ifd + 2 + 12 * i
            if struct.unpack("<H", good[at:at + 2])[0] == tag:
                return at
        raise KeyError(tag)

    def patched(at, fmt, *v):
        return good[:at] + struct.pack(fmt, *v) + good[at + struct.calcsize(fmt):]

    raises(b"", "no TIFF signature")
    raises(b"GIF89a" + bytes(20), "no TIFF signature")
    raises(good[:6], "header runs past")
    raises(patched(4, "<I", len(good) + 10), "offset of the first IFD .* past the end")
    raises(good[:ifd + 20], "first IFD .* runs past the end")
    raises(patched(entry(273) + 8, "<I", len(good) + 100), "values of tag 273 lie at an offset past the end")        # three strips: the offsets lie outside
    raises(patched(entry(273) + 4, "<I", 0x7fffffff), "count of tag 273 .* overflows")
    raises(patched(entry(258) + 4, "<I", 0xffffffff), "count of tag 258 .* overflows")
    one = _file()                                                        # one strip: offset and count are inline
    ifd1, = struct.unpack("<I", one[4:8])
    n1, = struct.unpack("<H", one[ifd1:ifd1 + 2])
    at279 = next(ifd1 + 2 + 12 * i for i in range(n1) if struct.unpack("<H", one[ifd1 + 2 + 12 * i:ifd1 + 4 + 12 * i])[0] == 279)
    raises(one[:at279 + 8] + struct.pack("<I", len(one)) + one[at279 + 12:], "strip 0 .* lies outside the file")
    raises(_file(rows_per_strip=2, extra={273: (R.LONG, [8, 26]), 279: (R.LONG, [18, 18])}), "2 strip offsets and 2 byte counts for the 3 strips")
    raises(_file(extra={278: (R.SHORT, [0])}), "RowsPerStrip is 0")
    raises(_file(extra={256: None}), "no ImageWidth")
    raises(_file(extra={256: (R.SHORT, [0])}), "zero width")
    raises(_file(extra={273: None}), "no StripOffsets")
    raises(R.assemble(_gray(), 9, 8, 1, 3), "palette image without a ColorMap")
    raises(_file(compression=R.ADOBE_DEFLATE, streams={0: b"\x78\x9d" + bytes(4)}), "corrupt zlib header")
    raises(_file(compression=R.ADOBE_DEFLATE, streams={0: b"\x78"}), "no zlib header")
    with pytest.raises(MafError, match="no files"):
        T.decode([], device="cuda:0")


def test_decode_names_the_file(tmp_path):
    p = tmp_path / "x.tif"
    p.write_bytes(b"not a tiff file")
    with pytest.raises(MafError, match=r"file 1 \(.*x\.tif\): tiff: no TIFF signature"):
        T.decode([_file(), str(p)], device="cuda:0")


def test_blob_layout_and_struct_sizes(cases):
    pick = ["lzw_rgb_noise_be_pred2_rps7", "palette4_5x7", "deflate_pred2_three_strips", "lzw_gray_1x1", "palette8_16x16_be"]
    datas = [cases["file_" + n].tobytes() for n in pick]
    infos = [T.parse(d) for d in datas]
    hdr, images, strips, palette = T.build_blob(infos)
    buf = np.full(int(hdr["total_bytes"]), 0xAA, np.uint8)
    T.fill_blob(buf, hdr, images, strips, palette, datas, infos)
    so = int(hdr["stream_off"])
    rows = ns = npal = 0
    for k, (d, im, info) in enumerate(zip(datas, images, infos)):
        deflate = info.compression in (8, 32946)
        assert int(im["rows_off"]) == rows and rows % 16 == 0 and int(im["out_off"]) % 16 == 0
        assert (int(im["first_strip"]), int(im["n_strips"])) == (ns, len(info.strips)) and int(im["rows_per_strip"]) == info.rows_per_strip <= info.height
        for j, (s, e) in enumerate(info.strips):
            sp = strips[ns + j]
            assert buf[so + int(sp["src_begin"]):so + int(sp["src_end"])].tobytes() == d[s + (2 if deflate else 0):e]      # a Deflate strip without its zlib header
            y0 = j * info.rows_per_strip
            assert int(sp["dst_off"]) == rows + y0 * info.row_bytes and int(sp["dst_bytes"]) == min(info.rows_per_strip, info.height - y0) * info.row_bytes
            assert int(sp["image"]) == k and int(sp["compression"]) == (8 if deflate else info.compression)
        if info.palette is not None:
            assert int(im["pal"]) == npal
            e = palette[npal:npal + len(info.palette)]
            assert np.array_equal(e[:, :3], info.palette[:, ::-1]) and not e[:, 3].any()
            npal += len(info.palette)
        ns += len(info.strips)
        rows += (info.height * info.row_bytes + 15) // 16 * 16
    assert (int(hdr["n_images"]), int(hdr["n_strips"]), int(hdr["n_palette"])) == (len(pick), ns, npal) == (5, ns, 16 + 256)
    assert int(hdr["rows_bytes"]) == rows and int(hdr["out_bytes"]) >= sum(3 * i.width * i.height for i in infos)
    end = so + int(strips[-1]["src_end"])
    assert int(hdr["total_bytes"]) - end >= T.STREAM_PAD and not buf[end:].any() and int(hdr["stream_bytes"]) % 8 == 0
    assert all(int(hdr[k]) % 16 == 0 for k in ("images_off", "strips_off", "palette_off", "stream_off"))
    assert (T.HEADER_DT.itemsize, T.IMAGE_DT.itemsize, T.STRIP_DT.itemsize) == (80, 64, 40)
    L = lib.load()                                                    # the built library: a missing one raises
    T._bind(L)
    sizes = (ctypes.c_int32 * 3)()
    lib.check(L.maf_tiff_struct_sizes(sizes))
    assert list(sizes) == [T.HEADER_DT.itemsize, T.IMAGE_DT.itemsize, T.STRIP_DT.itemsize]


_CTYPES = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int32_t*": ctypes.POINTER(ctypes.c_int32)}


def _header_prototypes(text):
    """name -> (restype, argtypes) of every function prototype of a C header: a scalar by its type, the int32_t* of the size query as it is
    (the binding type-checks it), every other pointer (and the stream handle) as void*."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^\s*(int|void)\s+(maf_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        args = []
        for p in params.split(","):
            words = p.replace("*", " * ").split()
            typ = " ".join(w for w in words[:-1] if w != "const").replace(" *", "*")
            if name == "maf_tiff_struct_sizes" and typ == "int32_t*":
                args.append(_CTYPES[typ])
            elif typ.endswith("*") or typ == "maf_tiff_stream_t":
                args.append(ctypes.c_void_p)
            else:
                args.append(_CTYPES[typ])
        out[name] = (_CTYPES[ret], args)
    return out


def test_binding_equals_the_header():
    with open(os.path.join(ROOT, "include", "mafyolo_tiff.h")) as f:
        text = f.read()
    protos = _header_prototypes(text)
    assert sorted(protos) == ["maf_tiff_decode", "maf_tiff_struct_sizes"] == sorted(T.PROTOTYPES)
    for name, (res, args) in protos.items():
        assert T.PROTOTYPES[name] == (res, args), name
    assert len(protos["maf_tiff_decode"][1]) == 6
    L = T._bind(lib.load())
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the constants the binding repeats
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(MAF_TIFF_\w+)\s+(\d+)\b", text)}
    assert [defs["MAF_TIFF_ST_" + n] for n in ("INPUT_EXHAUSTED", "LZW_BAD_CODE", "LZW_TABLE_FULL", "PACKBITS_OVERRUN")] == [b for b, _ in T._STATUS_TEXT[:4]]
    assert (defs["MAF_TIFF_ST_INFLATE_SHIFT"], defs["MAF_TIFF_STREAM_PAD"], defs["MAF_TIFF_MAX_SIDE"]) == (T.STATUS_INFLATE_SHIFT, T.STREAM_PAD, T.MAX_SIDE) and defs["MAF_TIFF_MAX_STRIP_ROWS_BYTES"] == T.MAX_STRIP_ROWS_BYTES
    assert [defs["MAF_TIFF_COMP_" + n] for n in ("NONE", "LZW", "DEFLATE", "PACKBITS")] == [T.COMP_NONE, T.COMP_LZW, T.COMP_ADOBE_DEFLATE, T.COMP_PACKBITS]
    # outside the signature table
    with open(os.path.join(ROOT, "include", "mafyolo_hip.h")) as f:
        assert "maf_tiff" not in f.read()
    assert not [n for n in lib.EXPORTS if "tiff" in n] and not [n for n in lib.TYPED_POINTERS if "tiff" in n]


def test_router_without_the_flag_is_unchanged(cases):
    d = cases["file_gray8_w1"].tobytes()
    be = cases["file_palette8_16x16_be"].tobytes()
    assert d[:4] == b"II*\0" and be[:4] == b"MM\0*"
    assert F.kind(d) is None and F.kind(d, webp=True, lossy=True) is None and F.kind(d, True, True) is None
    assert F.kind(d, tiff=True) == F.kind(be, tiff=True) == F.kind(be, True, True, True) == "tiff"
    assert F.kind(b"II+\0" + bytes(12), tiff=True) is None                # BigTIFF has another signature: not routed
    assert F.kind(P.SIGNATURE + bytes(8), tiff=True) == "png" and F.kind(b"\xff\xd8\xff", tiff=True) == "jpeg" and F.kind(b"RIFF\0\0\0\0WEBP", tiff=True) is None
    for kw in (dict(), dict(webp=True), dict(webp=True, lossy=True)):
        with pytest.raises(MafError, match="file 1: neither a JPEG nor a PNG signature"):
            F.decode([b"\xff\xd8\xff", d], device="cuda:0", **kw)
    # the router says which inputs went to tiff.decode when that call refuses one (the files are parsed before the device is touched)
    with pytest.raises(T.TiffUnsupported, match=r"file 1: tiff: FillOrder 2 .* \[tiff files of this call are inputs \[0, 1\]\]"):
        F.decode([d, _file(extra={266: (R.SHORT, [2])})], device="cuda:0", tiff=True)


def test_router_sniffs_and_keeps_the_order(monkeypatch, cases, golden):
    tiff_le, tiff_be = cases["file_gray8_w1"].tobytes(), cases["file_palette8_16x16_be"].tobytes()
    wl = golden("webp_lossy_cases")
    lossy_file = wl["file_" + str(wl["names"][0])].tobytes()
    wz = golden("webp_cases")
    webp_file = wz["file_" + str(wz["names"][0])].tobytes()
    png_file = golden("png_cases")["file_rgb8_3x5"].tobytes()
    jz = golden("jpeg_cases")
    jpeg_file = jz["file_" + str(jz["names"][0])].tobytes()
    calls = []

    def fake_jpeg(files, device=None, stream=None, ignore_orientation=False, check=True, progressive=False):
        calls.append(("jpeg", len(files), ignore_orientation, progressive, device, stream))
        return ["j%d" % i for i in range(len(files))]

    def fake_png(files, device=None, stream=None, check=True):
        calls.append(("png", len(files), device, stream))
        return ["p%d" % i for i in range(len(files))]

    def fake_webp(files, device=None, stream=None, check=True, ignore_orientation=False):
        calls.append(("webp", len(files), ignore_orientation, device, stream))
        return ["w%d" % i for i in range(len(files))]

    def fake_lossy(files, device=None, stream=None, check=True, ignore_orientation=False):
        calls.append(("webp_lossy", len(files), ignore_orientation, device, stream))
        return ["l%d" % i for i in range(len(files))]

    def fake_tiff(files, device=None, stream=None, check=True, ignore_orientation=False):
        calls.append(("tiff", len(files), ignore_orientation, device, stream))
        assert all(F.kind(f, tiff=True) == "tiff" for f in files)
        return ["t%d" % i for i in range(len(files))]

    monkeypatch.setattr(J, "decode", fake_jpeg)
    monkeypatch.setattr(P, "decode", fake_png)
    monkeypatch.setattr(W, "decode", fake_webp)
    monkeypatch.setattr(WL, "decode", fake_lossy)
    monkeypatch.setattr(T, "decode", fake_tiff)
    got = F.decode([tiff_le, lossy_file, webp_file, png_file, tiff_be, jpeg_file, lossy_file, jpeg_file, png_file, tiff_le], device="cuda:0", stream="s",
                   progressive=True, ignore_orientation=True, webp=True, lossy=True, tiff=True)
    assert got == ["t0", "l0", "w0", "p0", "t1", "j0", "l1", "j1", "p1", "t2"]
    assert sorted(calls) == [("jpeg", 2, True, True, "cuda:0", "s"), ("png", 2, "cuda:0", "s"), ("tiff", 3, True, "cuda:0", "s"), ("webp", 1, True, "cuda:0", "s"),
                             ("webp_lossy", 2, True, "cuda:0", "s")]
    calls.clear()
    assert F.decode([tiff_be, jpeg_file], tiff=True) == ["t0", "j0"] and sorted(calls) == [("jpeg", 1, False, False, None, None), ("tiff", 1, False, None, None)]
    calls.clear()
    with pytest.raises(MafError, match="file 1: neither a JPEG nor a PNG signature"):      # without the flag a TIFF file goes nowhere, as before
        F.decode([jpeg_file, tiff_be], webp=True, lossy=True)
    assert calls == []
