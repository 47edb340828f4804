"""No GPU: the header walk (maf-yolo_amd/bmp.py parse), the rule book, the hand assembler and the rewrite (tests/bmp_ref.py), the hand-written
binding, the host-side blob validation and the router; MPO files through frames.kind and jpeg.parse.

* bmp_ref equals the fixtures (tests/golden/bmp_cases.npz, written by tools/make_golden_bmp.py: Pillow's pixels) and, with Pillow, a fresh
  Pillow decode of every directly judged fixture and of files assembled or written by Pillow here;
* every fixture with a construct Pillow 12.2 reads differently from the rule (an odd RLE4 absolute run, an end of line on an empty row, an early
  end of bitmap) goes through bmp_ref.rewrite: the rewrite has none of the three left, the rule book gives the original's pixels for it, and so
  does Pillow;
* the rule book predicts the stored status word of every malformed fixture;
* parse reads every case; each unsupported kind is named in its BmpUnsupported; corrupt headers raise MafError; decode names the offending
  file before the device is touched;
* blob layout and alignment; the struct sizes equal maf_bmp_struct_sizes of the built library; a tampered blob (a bad offset, count or range)
  is rejected by maf_bmp_decode on the host, before any device pointer is used;
* the prototypes of include/mafyolo_bmp.h, read by regex, equal bmp.py's argtypes and restype; neither function is in lib.EXPORTS or
  mafyolo_hip.h;
* the router: without bmp=True a BMP file is refused exactly as before, with it the order is kept (fakes);
* an MPO file is 'jpeg' to frames.kind, and jpeg.parse reports its first frame.
"""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

import bmp_ref as R
from maf_yolo_amd import bmp as B, frames as F, jpeg as J, lib, png as P, tiff as T
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


needs_pillow = pytest.mark.skipif(_pillow() is None, reason="no Pillow: the judge of the rule book is absent")


@pytest.fixture(scope="module")
def cases(golden):
    return golden("bmp_cases")


def _names(z, key="names"):
    return [str(n) for n in z[key]]


def _pillow_bgr(d):
    return np.asarray(_pillow().open(io.BytesIO(d)).convert("RGB"))[..., ::-1]


PAL256 = np.random.default_rng(3).integers(0, 256, (256, 3), dtype=np.uint8)
IDX = np.random.default_rng(5).integers(0, 256, (6, 9))


def _file(bits=8, **kw):
    """A small good file; keywords go to the assembler."""
    if bits <= 8:
        kw.setdefault("palette", PAL256[:1 << bits])
        px = IDX & ((1 << bits) - 1)
    else:
        px = np.random.default_rng(6).integers(0, 256, (6, 9, bits // 8))
    return R.assemble(9, 6, bits, R.pack_rows(px, bits, kw.get("top_down", False)), **kw)


def _rle(rle4=False, **kw):
    return R.rle_file(9, 6, R.rle_records(IDX & (15 if rle4 else 255), rle4), rle4, PAL256[:16 if rle4 else 256], **kw)


def test_rule_book_equals_the_fixtures(cases):
    names = _names(cases)
    assert len(names) >= 40
    for word in (["bi1_w%d" % w for w in (1, 7, 8, 9, 31, 32, 33)] + ["bi4_w%d" % w for w in (1, 2, 3, 7, 8, 9)] + ["bi8_w%d" % w for w in (1, 2, 3, 4, 5)] +
                 ["bgr24_w%d" % w for w in (1, 2, 3, 4, 5)] + ["bgrx32_plain", "bgrx32_bitfields_header40", "bgra32_bitfields_header108_alpha", "bi8_h1",
                                                                "bi4_top_down", "bgr24_13x3_top_down", "bi8_header12_os2", "bi8_header52", "bgr24_header56", "bi4_header64",
                                                                "bi1_header108", "bgr24_header124", "bi8_colors2_out_of_palette", "bi8_gray_palette", "bi8_gap_before_data"] +
                 [k + n for k in ("rle8_", "rle4_") for n in ("runs_of_1_and_255", "absolute_3_4_5", "absolute_254_255_longer_than_a_window", "delta_mid_row_and_at_row_end",
                                                              "empty_row_eol", "early_eob", "data_after_eob", "no_eol_before_eob", "delta_operands_straddle_a_window",
                                                              "absolute_header_on_the_last_lane", "absolute_payload_straddles_a_window", "noise_70x50", "single_colour_40x6",
                                                              "1x1")]):
        assert word in names, word
    for n in names:
        d = cases["file_" + n].tobytes()
        bgr, plane, st = R.decode_stages(d)
        assert st == 0 and bgr.dtype == np.uint8 and np.array_equal(bgr, cases["bgr_" + n]), n
        assert (plane is not None) == n.startswith("rle"), n
        assert str(cases["judge_" + n]) == ("rewrite" if R.departs(d) else "direct"), n


def test_the_cases_reach_their_edges(cases):
    """The fixtures are what their names say."""
    def hd(n):
        return R.read_header(cases["file_" + n].tobytes())

    assert [hd(n)["header"] for n in ("bi8_header12_os2", "bi8_w1", "bi8_header52", "bgr24_header56", "bi4_header64", "bi1_header108", "bgr24_header124")] == list(R.HEADER_SIZES)
    assert hd("bi4_top_down")["top_down"] and hd("bgr24_13x3_top_down")["top_down"] and not hd("bi8_w1")["top_down"]
    assert hd("bi8_colors2_out_of_palette")["colors"] == 2 and hd("bgrx32_bitfields_header40")["compression"] == R.BITFIELDS
    d = cases["file_bi8_colors2_out_of_palette"].tobytes()
    assert np.frombuffer(d, np.uint8, 4 * 12, hd("bi8_colors2_out_of_palette")["offset"]).max() >= 2
    assert hd("bi8_gap_before_data")["offset"] == 14 + 40 + 1024 + 10
    rows = np.frombuffer(cases["file_bgrx32_plain"].tobytes(), np.uint8, 4 * 5 * 4, hd("bgrx32_plain")["offset"]).reshape(-1, 4)
    assert rows[:, 3].min() > 0                                                        # non-zero 4th bytes
    for rle4 in (False, True):
        k = "rle4_" if rle4 else "rle8_"

        def recs(n):
            d = cases["file_" + k + n].tobytes()
            return R.records(d[R.read_header(d)["offset"]:], rle4)

        r = recs("delta_operands_straddle_a_window")
        assert [(o, rec[0]) for o, rec in r if rec[0] == "delta"] == [(126, "delta")]    # its operands are bytes 128 and 129
        r = recs("absolute_header_on_the_last_lane")
        assert (126, "abs") in [(o, rec[0]) for o, rec in r]
        o, rec = next((o, rec) for o, rec in recs("absolute_payload_straddles_a_window") if rec[0] == "abs")
        assert o + 2 < 128 < o + 2 + len(rec[2])
        assert any(rec[0] == "abs" and 2 + len(rec[2]) > 128 for _, rec in recs("absolute_254_255_longer_than_a_window"))
        d = cases["file_" + k + "noise_70x50"].tobytes()
        assert len(d) - R.read_header(d)["offset"] > 10 * 128
        assert recs("data_after_eob")[-1][1] == ("eob",) and recs("full_image_without_eob")[-1][1] is None
    assert R.departs(cases["file_rle4_absolute_3_4_5"].tobytes()) == ["odd_rle4_absolute"] and R.departs(cases["file_rle8_absolute_3_4_5"].tobytes()) == []
    assert R.departs(cases["file_rle8_empty_row_eol"].tobytes()) == ["empty_row_eol"] and R.departs(cases["file_rle8_early_eob"].tobytes()) == ["early_eob"]


@needs_pillow
def test_rule_book_equals_pillow_on_the_directly_judged_cases(cases):
    n_direct = 0
    for n in _names(cases):
        if str(cases["judge_" + n]) != "direct":
            continue
        d = cases["file_" + n].tobytes()
        want = _pillow_bgr(d)
        assert np.array_equal(R.decode(d), want) and np.array_equal(cases["bgr_" + n], want), n
        n_direct += 1
    assert n_direct >= 40


@needs_pillow
def test_rule_book_through_the_rewrite(cases):
    seen = set()
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        why = R.departs(d)
        if not why:
            continue
        assert str(cases["judge_" + n]) == "rewrite", n
        seen.update(why)
        d2 = R.rewrite(d)
        assert R.departs(d2) == [] and d2[:R.read_header(d)["offset"]] == d[:R.read_header(d)["offset"]], n
        bgr, plane, st = R.decode_stages(d)
        bgr2, plane2, st2 = R.decode_stages(d2)
        assert st == st2 == 0 and np.array_equal(bgr2, bgr) and np.array_equal(plane2, plane), n
        assert np.array_equal(_pillow_bgr(d2), bgr) and np.array_equal(cases["bgr_" + n], bgr), n
        assert B.supported(d) and B.supported(d2), n
    assert seen == {"odd_rle4_absolute", "empty_row_eol", "early_eob"}
    # the rewrite of a file without such a construct keeps its records
    d = cases["file_rle8_noise_70x50"].tobytes()
    assert R.rewrite(d) == d


@needs_pillow
def test_rule_book_equals_pillow_on_fresh_files():
    Image = _pillow()
    rng = np.random.default_rng(12)
    for bits in (1, 4, 8, 24, 32):
        for w in list(range(1, 18)) + [31, 32, 33, 64, 65]:
            for top_down in (False, True):
                h = 1 + w % 4
                px = rng.integers(0, 1 << min(bits, 8), (h, w) if bits <= 8 else (h, w, bits // 8))
                colors = None if bits > 8 else int(rng.integers(3 if bits > 1 else 2, (1 << bits) + 1))
                pal = None if bits > 8 else rng.integers(0, 256, (colors, 3), dtype=np.uint8)
                d = R.assemble(w, h, bits, R.pack_rows(px, bits, top_down), header=(40, 108, 124, 56)[w % 4], top_down=top_down, palette=pal, gap=(w % 3) * 2)
                assert np.array_equal(R.decode(d), _pillow_bgr(d)), (bits, w, top_down)
                info = B.parse(d)
                assert (info.width, info.height, info.bits, info.top_down) == (w, h, bits, top_down) and B.supported(d)
    for rle4 in (False, True):
        for w, h in ((1, 1), (2, 3), (17, 5), (64, 3), (129, 4), (300, 2)):
            plane = rng.integers(0, 16 if rle4 else 256, (h, w))
            plane[h // 2, w // 3:] = 1
            for kw in (dict(), dict(abs_max=4), dict(eol_last=True)):
                d = R.rle_file(w, h, R.rle_records(plane, rle4, **kw), rle4, PAL256[:16 if rle4 else 200])
                assert R.departs(d) == [] and np.array_equal(R.decode(d), _pillow_bgr(d)) and B.supported(d), (rle4, w, h, kw)
                assert np.array_equal(R.decode_stages(d)[1], plane)
    y, x = np.mgrid[0:23, 0:31]
    rgb = np.stack([(x * 7 + y) & 255, (x + y * 3) & 255, (x * y) & 255], -1).astype(np.uint8)
    for mode in ("1", "L", "P", "RGB", "RGBA"):
        buf = io.BytesIO()
        Image.fromarray(rgb).convert(mode).save(buf, "BMP")
        d = buf.getvalue()
        assert B.supported(d) and np.array_equal(R.decode(d), _pillow_bgr(d)), mode


def test_rule_book_predicts_the_malformed_status(cases):
    want = {"rle8_ends_without_eob": 1, "rle8_absolute_payload_cut": 1, "rle4_delta_operands_cut": 1, "rle8_run_past_row": 2, "rle4_absolute_run_past_row": 2,
            "rle8_full_row_without_eol": 2, "rle4_delta_above_the_image": 4, "rle8_delta_right_of_the_row": 4, "rle8_run_past_row_in_the_second_window": 2}
    assert sorted(_names(cases, "bad_names")) == sorted(want)
    for n, w in want.items():
        d = cases["badfile_" + n].tobytes()
        assert B.supported(d), n                                      # the headers are intact: only the decoder can tell
        bgr, plane, st = R.decode_stages(d)
        assert st == int(cases["badstatus_" + n]) == w, n
    # a run past its row's end is clamped there, and what follows the fault is index 0
    _, plane, _ = R.decode_stages(cases["badfile_rle8_run_past_row"].tobytes())
    assert plane[0].tolist() == [9] * 5 + [200] * 3 and not plane[1:].any()
    _, plane, _ = R.decode_stages(cases["badfile_rle4_delta_above_the_image"].tobytes())
    assert plane[0].tolist() == [1, 2, 1, 0, 0, 0, 0, 0] and not plane[1:].any()
    assert (B.STATUS_INPUT_EXHAUSTED, B.STATUS_RUN_PAST_ROW, B.STATUS_DELTA_PAST_IMAGE) == (R.ST_INPUT_EXHAUSTED, R.ST_RUN_PAST_ROW, R.ST_DELTA_PAST_IMAGE) == (1, 2, 4)
    assert B.status_text(6) == "an RLE run that crosses the end of its row, an RLE delta that leaves the image"
    assert B.status_text(1) == "RLE data that ends with no end of bitmap before the last row is complete"


def test_parse_reads_every_case(cases):
    for n in _names(cases) + _names(cases, "bad_names"):
        d = cases[("file_" if "file_" + n in cases else "badfile_") + n].tobytes()
        hd = R.read_header(d)
        info = B.parse(d)
        assert (info.width, info.height, info.bits, info.compression, info.top_down, info.header_size) == (
            hd["width"], hd["height"], hd["bits"], hd["compression"], hd["top_down"], hd["header"]), n
        rle = hd["compression"] in (R.RLE8, R.RLE4)
        stride = (info.width * info.bits + 31) // 32 * 4
        assert info.row_bytes == (0 if rle else stride) and info.data == (hd["offset"], len(d) if rle else hd["offset"] + info.height * stride), n
        if info.bits <= 8:
            colors = hd["colors"] or 1 << info.bits
            want = np.frombuffer(d, np.uint8, colors * hd["entry"], 14 + hd["header"]).reshape(colors, hd["entry"])[:, :3]
            assert info.colors == colors and np.array_equal(info.palette, want), n
        else:
            assert info.palette is None and info.colors == 0, n


def test_unsupported_kinds_are_named():
    def raises(d, word):
        with pytest.raises(B.BmpUnsupported, match=word):
            B.parse(d)
        assert not B.supported(d)

    for bits in (1, 4, 8, 24, 32):
        assert B.supported(_file(bits)) and B.supported(_file(bits, top_down=True))
    assert B.supported(_rle()) and B.supported(_rle(True))
    px16 = np.zeros((6, 9, 2), np.uint8)
    raises(R.assemble(9, 6, 16, R.pack_rows(px16, 16)), "16-bit files")
    raises(R.assemble(9, 6, 16, R.pack_rows(px16, 16), compression=R.BITFIELDS, masks=(0xF800, 0x7E0, 0x1F)), "16-bit files")
    raises(_file(32, compression=R.BITFIELDS, masks=(0xFF, 0xFF00, 0xFF0000)), "BITFIELDS layout of 32 bits with the masks 0xff 0xff00 0xff0000")
    raises(_file(32, header=108, compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF), alpha=0xFF), "BITFIELDS layout .* alpha 0xff ")
    raises(_file(32, header=124, compression=R.BITFIELDS, masks=(0, 0, 0)), "BITFIELDS layout")
    raises(_file(24, compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF)), "BITFIELDS layout of 24 bits")
    raises(_file(24, compression=4), r"compression 4 \(BI_JPEG\)")
    raises(_file(24, compression=5), r"compression 5 \(BI_PNG\)")
    raises(_file(24, compression=6), "compression 6")
    raises(_file(24, header=64, compression=3), "compression 3 is not supported")      # OS/2 v2: Huffman 1D
    raises(_file(8, compression=R.RLE4), "BI_RLE4 at 8 bits")
    raises(_file(4, compression=R.RLE8), "BI_RLE8 at 4 bits")
    raises(_rle(top_down=True), "top-down RLE")
    raises(_rle(True, top_down=True), "top-down RLE")
    raises(_file(4, palette=PAL256[:17], colors=17), "palette of 17 colors at 4 bits")
    raises(_file(1, palette=PAL256[:3], colors=3), "palette of 3 colors at 1 bits")
    for hs in (16, 48, 128, 0):
        d = bytearray(_file(8))
        d[14:18] = struct.pack("<I", hs)
        raises(bytes(d), "DIB header of %d bytes" % hs)
    raises(_rle(gap=1), "RLE data at an odd offset")
    assert B.supported(_rle(gap=2))
    raises(_file(8, planes=3), "3 planes")
    raises(R.assemble(9, 6, 2, bytes(24), palette=PAL256[:4]), "2 bits per pixel")
    raises(R.assemble(9, 6, 64, bytes(6 * 72)), "64 bits per pixel")
    raises(R.assemble(70000, 1, 8, bytes(70000), palette=PAL256), "70000 x 1 is beyond")
    raises(R.assemble(65535, 20000, 24, b""), "beyond the 2 GiB of rows")
    raises(_file(8, offset=14 + 40), "bfOffBits 54. inside the headers or the palette")
    raises(_file(32, compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF), offset=14 + 40 + 4), "inside the headers")
    gray16 = np.repeat(np.arange(16, dtype=np.uint8)[:, None], 3, 1)
    raises(_file(4, palette=gray16), "gray ramp palette of 16 entries at 4 bits")
    raises(_file(8, palette=np.array([[0, 0, 0], [255, 255, 255]], np.uint8)), "gray ramp palette of 2 entries at 8 bits")
    with pytest.raises(B.BmpUnsupported, match=r"file 1: bmp: 16-bit files"):
        B.decode([_file(), R.assemble(9, 6, 16, R.pack_rows(px16, 16))], device="cuda:0")      # parsed before the device is touched
    assert issubclass(B.BmpUnsupported, MafError)


def test_corrupt_headers_raise_maferror():
    good = _file(8)
    assert B.supported(good)

    def raises(d, word):
        with pytest.raises(MafError, match=word) as e:
            B.parse(d)
        assert not isinstance(e.value, B.BmpUnsupported) and not B.supported(d)

    def patched(at, fmt, *v):
        return good[:at] + struct.pack(fmt, *v) + good[at + struct.calcsize(fmt):]

    raises(b"", "no BM signature")
    raises(b"GIF89a" + bytes(20), "no BM signature")
    raises(good[:16], "file header runs past")
    raises(good[:40], "DIB header .40 bytes. runs past")
    raises(patched(18, "<i", 0), "zero or negative width")
    raises(patched(18, "<i", -9), "zero or negative width")
    raises(patched(22, "<i", 0), "zero height")
    raises(good[:54 + 1000], "palette .256 entries. runs past")
    raises(patched(10, "<I", len(good) + 1), "bfOffBits .* lies past the end")
    raises(good[:-1], "truncated pixel data")
    raises(_file(24)[:-3], "truncated pixel data")
    raises(_file(32, compression=R.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF))[:60], "BITFIELDS masks run past")
    with pytest.raises(MafError, match="no files"):
        B.decode([], device="cuda:0")
    Image = _pillow()
    if Image is not None:                                                # Pillow raises once a pixel is missing (it forgives the last row's padding; parse does not)
        with pytest.raises(OSError, match="truncated"):
            Image.open(io.BytesIO(good[:-4])).load()


def test_decode_names_the_file(tmp_path):
    p = tmp_path / "x.bmp"
    p.write_bytes(b"not a bmp file")
    with pytest.raises(MafError, match=r"file 1 \(.*x\.bmp\): bmp: no BM signature"):
        B.decode([_file(), str(p)], device="cuda:0")


PICK = ["rle8_noise_70x50", "bi4_w7", "bgr24_w3", "rle4_absolute_3_4_5", "bi8_colors2_out_of_palette", "bgrx32_plain", "bi1_header12_os2"]


def _blob(cases, edit=None):
    datas = [cases["file_" + n].tobytes() for n in PICK]
    infos = [B.parse(d) for d in datas]
    hdr, images, rle, palette = B.build_blob(infos)
    buf = np.full(int(hdr["total_bytes"]), 0xAA, np.uint8)
    B.fill_blob(buf, hdr, images, rle, palette, datas, infos)
    if edit is not None:                                                # the tampered tables go where the good ones lay
        at = int(hdr["images_off"]), int(hdr["rle_off"])
        edit(hdr, images, rle)
        buf[:B.HEADER_DT.itemsize] = np.frombuffer(hdr.tobytes(), np.uint8)
        buf[at[0]:at[0] + images.nbytes] = images.view(np.uint8)
        buf[at[1]:at[1] + rle.nbytes] = rle.view(np.uint8)
    return buf, hdr, images, rle, palette, datas, infos


def test_blob_layout_and_struct_sizes(cases):
    buf, hdr, images, rle, palette, datas, infos = _blob(cases)
    so = int(hdr["stream_off"])
    planes = npal = outb = at = 0
    for k, (d, im, info) in enumerate(zip(datas, images, infos)):
        s, e = info.data
        assert int(im["src_begin"]) == at and at % 16 == 0 and int(im["src_end"]) - at == e - s
        assert buf[so + at:so + int(im["src_end"])].tobytes() == d[s:e]
        assert not buf[so + int(im["src_end"]):so + (int(im["src_end"]) + 15) // 16 * 16].any()          # the gap up to the next file is zero
        assert int(im["out_off"]) == outb and outb % 16 == 0
        is_rle = info.compression in (1, 2)
        assert int(im["compression"]) == (info.compression if is_rle else 0) and int(im["row_bytes"]) == info.row_bytes and int(im["top_down"]) == info.top_down
        if is_rle:
            assert int(im["plane_off"]) == planes
            planes += (info.width * info.height + 15) // 16 * 16
        if info.palette is not None:
            assert (int(im["pal"]), int(im["n_colors"])) == (npal, info.colors)
            e4 = palette[npal:npal + info.colors]
            assert np.array_equal(e4[:, :3], info.palette) and not e4[:, 3].any()
            npal += info.colors
        else:
            assert (int(im["pal"]), int(im["n_colors"])) == (0, 0)
        at = (int(im["src_end"]) + 15) // 16 * 16
        outb += (3 * info.width * info.height + 15) // 16 * 16
    assert rle.tolist() == [0, 3] and (int(hdr["n_images"]), int(hdr["n_rle"]), int(hdr["n_palette"])) == (len(PICK), 2, npal) == (7, 2, 256 + 16 + 16 + 2 + 2)
    assert int(hdr["planes_bytes"]) == planes and int(hdr["out_bytes"]) == outb
    assert int(hdr["stream_bytes"]) == at + B.STREAM_PAD and int(hdr["total_bytes"]) == so + at + B.STREAM_PAD and not buf[so + at:int(hdr["total_bytes"])].any()
    assert all(int(hdr[k]) % 16 == 0 for k in ("images_off", "rle_off", "palette_off", "stream_off"))
    assert (B.HEADER_DT.itemsize, B.IMAGE_DT.itemsize) == (80, 64)
    L = lib.load()                                                    # the built library: a missing one raises
    B._bind(L)
    sizes = (ctypes.c_int32 * 2)()
    lib.check(L.maf_bmp_struct_sizes(sizes))
    assert list(sizes) == [B.HEADER_DT.itemsize, B.IMAGE_DT.itemsize]
    assert B._library() is L


def _set(table, field, value, at=0):
    def edit(hdr, images, rle):
        t = dict(hdr=hdr, images=images, rle=rle)[table]
        if table == "hdr":
            t[field] = value
        elif table == "rle":
            t[at] = value
        else:
            t[field][at] = value(int(t[field][at])) if callable(value) else value
    return edit


@pytest.mark.parametrize("what, edit", [
    ("1 to 65535 images", _set("hdr", "n_images", 0)),
    ("1 to 65535 images", _set("hdr", "n_images", 70000)),
    ("blob size out of range", _set("hdr", "total_bytes", -16)),
    ("RLE image count out of range", _set("hdr", "n_rle", 8)),
    ("palette entry count out of range", _set("hdr", "n_palette", 256 * 7 + 1)),
    ("section lies outside the blob", _set("hdr", "images_off", 1 << 24)),
    ("section lies outside the blob", _set("hdr", "palette_off", 88)),
    ("section lies outside the blob", _set("hdr", "stream_bytes", 1 << 24)),
    ("section lies outside the blob", _set("hdr", "stream_bytes", 32)),
    ("output buffer sizes out of range", _set("hdr", "out_bytes", 0)),
    ("output buffer sizes out of range", _set("hdr", "planes_bytes", 1 << 31)),
    ("bad image size", _set("images", "w", 0, 1)),
    ("bad image size", _set("images", "h", 65536, 2)),
    ("bits per pixel is 1, 4, 8, 24 or 32", _set("images", "bits", 16, 2)),
    ("compression does not go with the bit depth", _set("images", "compression", 1, 1)),
    ("compression does not go with the bit depth", _set("images", "compression", 3, 2)),
    ("top_down is 0, or 1 on uncompressed rows", _set("images", "top_down", 1, 0)),
    ("top_down is 0, or 1 on uncompressed rows", _set("images", "top_down", 2, 1)),
    ("data lies outside the stream section", _set("images", "src_end", 1 << 20, 0)),
    ("data lies outside the stream section", _set("images", "src_begin", -16, 0)),
    ("data lies outside the stream section", _set("images", "src_begin", lambda v: v + 8, 1)),
    ("frame lies outside the output buffer", _set("images", "out_off", 1 << 20, 6)),
    ("frame lies outside the output buffer", _set("images", "out_off", 8, 0)),
    ("row_bytes or the data size does not match", _set("images", "row_bytes", 8, 1)),
    ("row_bytes or the data size does not match", _set("images", "h", 4, 2)),
    ("row_bytes or the data size does not match", _set("images", "w", 9, 5)),
    ("an RLE image has no row_bytes", _set("images", "row_bytes", 4, 0)),
    ("index plane lies outside the planes buffer", _set("images", "plane_off", 1 << 20, 3)),
    ("index plane lies outside the planes buffer", _set("images", "w", 71, 0)),
    ("RLE list does not name the RLE images in order", _set("rle", None, 1, 0)),
    ("RLE list does not name the RLE images in order", _set("rle", None, 0, 1)),
    ("RLE list entries that belong to no image", _set("images", "compression", 0, 3)),
    ("palette lies outside the palette section", _set("images", "n_colors", 17, 1)),
    ("palette lies outside the palette section", _set("images", "n_colors", 0, 4)),
    ("palette lies outside the palette section", _set("images", "pal", 291, 6)),
    ("24 or 32-bit image has no palette", _set("images", "n_colors", 2, 2)),
])
def test_c_abi_rejects_a_tampered_blob_before_the_device(cases, what, edit):
    """Every offset, count and range of the host copy is validated first: the device pointers below are never used."""
    if what.startswith("RLE list entries"):                             # an RLE image turned into an uncompressed one of the right size
        inner = edit

        def edit(hdr, images, rle):
            inner(hdr, images, rle)
            images["bits"][3], images["row_bytes"][3] = 8, 12
            images["src_end"][3] = images["src_begin"][3] + 24
            images["n_colors"][3] = 16
    buf = _blob(cases, edit)[0]
    L = B._bind(lib.load())
    rc = L.maf_bmp_decode(buf.ctypes.data, 4096, 8192, 12288, 16384, None)
    assert rc != 0
    assert what in L.maf_last_error().decode(), L.maf_last_error().decode()


def test_c_abi_rejects_null_and_misaligned_buffers(cases):
    buf = _blob(cases)[0]
    L = B._bind(lib.load())
    assert L.maf_bmp_decode(buf.ctypes.data, 4096, None, 12288, 16384, None) != 0 and "null" in L.maf_last_error().decode()
    assert L.maf_bmp_decode(buf.ctypes.data, 4096 + 8, 8192, 12288, 16384, None) != 0 and "aligned" in L.maf_last_error().decode()


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
            if name == "maf_bmp_struct_sizes" and typ == "int32_t*":
                args.append(_CTYPES[typ])
            elif typ.endswith("*") or typ == "maf_bmp_stream_t":
                args.append(ctypes.c_void_p)
            else:
                args.append(_CTYPES[typ])
        out[name] = (_CTYPES[ret], args)
    return out


def test_binding_equals_the_header():
    with open(os.path.join(ROOT, "include", "mafyolo_bmp.h")) as f:
        text = f.read()
    protos = _header_prototypes(text)
    assert sorted(protos) == ["maf_bmp_decode", "maf_bmp_struct_sizes"] == sorted(B.PROTOTYPES)
    for name, (res, args) in protos.items():
        assert B.PROTOTYPES[name] == (res, args), name
    assert len(protos["maf_bmp_decode"][1]) == 6
    L = B._bind(lib.load())
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the constants the binding repeats
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(MAF_BMP_\w+)\s+(\d+)\b", text)}
    assert [defs["MAF_BMP_ST_" + n] for n in ("INPUT_EXHAUSTED", "RUN_PAST_ROW", "DELTA_PAST_IMAGE")] == [b for b, _ in B._STATUS_TEXT]
    assert (defs["MAF_BMP_STREAM_PAD"], defs["MAF_BMP_MAX_SIDE"]) == (B.STREAM_PAD, B.MAX_SIDE)
    assert [defs["MAF_BMP_COMP_" + n] for n in ("RGB", "RLE8", "RLE4")] == [B.BI_RGB, B.BI_RLE8, B.BI_RLE4]
    # the struct fields, in order, against the numpy records
    for struct_name, dt in (("maf_bmp_header_t", B.HEADER_DT), ("maf_bmp_image_t", B.IMAGE_DT)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct_name, re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S).group(1)
        fields = []
        for typ, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
            fields += [(n.strip(), "<i4" if typ == "int32_t" else "<i8") for n in names.split(",")]
        assert fields == [(n, dt.fields[n][0].str) for n in dt.names], struct_name
    # outside the signature table
    with open(os.path.join(ROOT, "include", "mafyolo_hip.h")) as f:
        assert "maf_bmp" not in f.read()
    assert not [n for n in lib.EXPORTS if "bmp" in n] and not [n for n in lib.TYPED_POINTERS if "bmp" in n]


def test_router_without_the_flag_is_unchanged(cases):
    d = cases["file_bi8_w1"].tobytes()
    os2 = cases["file_bi8_header12_os2"].tobytes()
    assert d[:2] == os2[:2] == b"BM"
    assert F.kind(d) is None and F.kind(d, webp=True, lossy=True, tiff=True) is None and F.kind(d, True, True, True) is None
    assert F.kind(d, bmp=True) == F.kind(os2, bmp=True) == F.kind(os2, True, True, True, True) == "bmp"
    for n in _names(cases):
        assert F.kind(cases["file_" + n].tobytes(), bmp=True) == "bmp", n
    bad = bytearray(d)
    bad[14:18] = struct.pack("<I", 48)
    assert F.kind(bytes(bad), bmp=True) is None and F.kind(b"BM" + bytes(10), bmp=True) is None      # an unknown header size, a file too short to name one
    assert F.kind(P.SIGNATURE + bytes(8), bmp=True) == "png" and F.kind(b"\xff\xd8\xff", bmp=True) == "jpeg" and F.kind(b"II*\0" + bytes(8), bmp=True) is None
    for kw in (dict(), dict(webp=True), dict(webp=True, lossy=True, tiff=True)):
        with pytest.raises(MafError, match="file 1: neither a JPEG nor a PNG signature"):
            F.decode([b"\xff\xd8\xff", d], device="cuda:0", **kw)
    # the router says which inputs went to bmp.decode when that call refuses one (the files are parsed before the device is touched)
    with pytest.raises(B.BmpUnsupported, match=r"file 1: bmp: 16-bit files .* \[bmp files of this call are inputs \[0, 1\]\]"):
        F.decode([d, R.assemble(9, 6, 16, bytes(6 * 20))], device="cuda:0", bmp=True)


def test_router_sniffs_and_keeps_the_order(monkeypatch, cases, golden):
    bmp_a, bmp_b = cases["file_bi8_w1"].tobytes(), cases["file_rle4_1x1"].tobytes()
    mpo = cases["mpofile_mpo_two_frames_444"].tobytes()
    tz = golden("tiff_cases")
    tiff_file = tz["file_gray8_w1"].tobytes()
    png_file = golden("png_cases")["file_rgb8_3x5"].tobytes()
    jz = golden("jpeg_cases")
    jpeg_file = jz["file_" + str(jz["names"][0])].tobytes()
    calls = []

    def fake_jpeg(files, device=None, stream=None, ignore_orientation=False, check=True, progressive=False):
        calls.append(("jpeg", len(files), device, stream))
        return ["j%d" % i for i in range(len(files))]

    def fake_png(files, device=None, stream=None, check=True):
        calls.append(("png", len(files), device, stream))
        return ["p%d" % i for i in range(len(files))]

    def fake_tiff(files, device=None, stream=None, check=True, ignore_orientation=False):
        calls.append(("tiff", len(files), device, stream))
        return ["t%d" % i for i in range(len(files))]

    def fake_bmp(files, device=None, stream=None, check=True):
        calls.append(("bmp", len(files), device, stream))
        assert all(F.kind(f, bmp=True) == "bmp" for f in files)
        return ["b%d" % i for i in range(len(files))]

    monkeypatch.setattr(J, "decode", fake_jpeg)
    monkeypatch.setattr(P, "decode", fake_png)
    monkeypatch.setattr(T, "decode", fake_tiff)
    monkeypatch.setattr(B, "decode", fake_bmp)
    got = F.decode([bmp_a, mpo, png_file, tiff_file, bmp_b, jpeg_file, bmp_a], device="cuda:0", stream="s", tiff=True, bmp=True)
    assert got == ["b0", "j0", "p0", "t0", "b1", "j1", "b2"]
    assert sorted(calls) == [("bmp", 3, "cuda:0", "s"), ("jpeg", 2, "cuda:0", "s"), ("png", 1, "cuda:0", "s"), ("tiff", 1, "cuda:0", "s")]
    calls.clear()
    assert F.decode([bmp_b, jpeg_file], bmp=True) == ["b0", "j0"] and sorted(calls) == [("bmp", 1, None, None), ("jpeg", 1, None, None)]
    calls.clear()
    with pytest.raises(MafError, match="file 1: neither a JPEG nor a PNG signature"):      # without the flag a BMP file goes nowhere, as before
        F.decode([jpeg_file, bmp_a], webp=True, lossy=True, tiff=True)
    assert calls == []


def test_mpo_is_a_jpeg_whose_first_frame_is_parsed(cases):
    names = _names(cases, "mpo_names")
    assert len(names) >= 3
    for n in names:
        d = cases["mpofile_" + n].tobytes()
        want = cases["mpobgr_" + n]
        assert d[:2] == b"\xff\xd8" and b"MPF\0" in d[:4096] and d.count(b"\xff\xd8\xff") >= 2, n      # an APP2 MPF index, more JPEGs behind the first
        assert F.kind(d) == F.kind(d, True, True, True, True) == "jpeg", n
        info = J.parse(d)
        assert (info.height, info.width) == want.shape[:2], n
        assert J.supported(d), n
        Image = _pillow()
        if Image is not None:
            im = Image.open(io.BytesIO(d))
            assert im.format == "MPO" and im.n_frames >= 2
            im.seek(1)
            assert im.size != (info.width, info.height), n                                             # the second frame has another size
            assert np.array_equal(_pillow_bgr(d), want), n
