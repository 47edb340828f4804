"""No GPU: the RIFF walk and the 10 header bytes (maf-yolo_amd/webp_lossy.py parse), the rule book (tests/webp_lossy_ref.py), the hand-written
binding and the router.

* webp_lossy_ref equals the fixtures (tests/golden/webp_lossy_cases.npz, written by tools/make_golden_webp_lossy.py: Pillow's pixels and
  WebPDecodeYUV's planes) and, where Pillow has libwebp, a fresh Pillow decode of every fixture and of files written here;
* it predicts the stored status word of every malformed fixture; transcode without changes keeps the planes, and the bool writer round-trips;
* the two copies of the format's tables (tests/webp_lossy_tables.py, csrc/vp8_tables.h) hold the same numbers;
* parse classifies every refusal with its exception class and message, and decode names the offending file before the device is touched;
* blob layout and alignment; the struct sizes equal maf_vp8_struct_sizes of the built library;
* the prototypes of include/mafyolo_vp8.h, read by regex, equal webp_lossy.py's argtypes and restype; neither function is in lib.EXPORTS,
  mafyolo_hip.h or mafyolo_webp.h;
* the router: without lossy=True a lossy file is refused exactly as before, with it order and hand-on of the flags are right (fakes).
"""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

import webp_lossy_ref as R
import webp_lossy_tables as T
from maf_yolo_amd import frames as F, jpeg as J, lib, png as P, webp as W, webp_lossy as WL
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow():
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check("webp") else None


needs_pillow = pytest.mark.skipif(_pillow() is None, reason="Pillow without libwebp: the judge of the rule book is absent")


@pytest.fixture(scope="module")
def cases(golden):
    return golden("webp_lossy_cases")


def _names(z, key="names"):
    return [str(n) for n in z[key]]


def _file(cases, n="mixed_33x17_q90_m6"):
    return cases["file_" + n].tobytes()


def _chunk(cc, body):
    return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _riff(*chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _vp8x(w, h, flags=0):
    return _chunk(b"VP8X", bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))


def _payload(cases, n="mixed_33x17_q90_m6"):
    d = _file(cases, n)
    s, e = R.vp8_payload(d)
    return d[s:e]


def test_rule_book_equals_the_fixtures(cases):
    assert len(_names(cases)) >= 60
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        bgr, planes, st = R.decode_stages(d)
        assert st == 0, n
        assert bgr.dtype == np.uint8 and np.array_equal(bgr, cases["bgr_" + n]), n
        for key, p in zip("yuv", planes):
            assert p.dtype == np.uint8 and np.array_equal(p, cases[key + "_" + n]), (n, key)
        info = WL.parse(d)
        assert (info.height, info.width, 3) == bgr.shape and WL.supported(d), n


@needs_pillow
def test_fixtures_equal_a_fresh_pillow_decode(cases):
    Image = _pillow()
    for n in _names(cases):
        want = np.asarray(Image.open(io.BytesIO(cases["file_" + n].tobytes())).convert("RGBA"))[..., 2::-1]
        assert np.array_equal(cases["bgr_" + n], want), n
    for n in _names(cases, "bad_names"):
        with pytest.raises(Exception):
            Image.open(io.BytesIO(cases["badfile_" + n].tobytes())).convert("RGBA").load()


@needs_pillow
def test_rule_book_equals_pillow_on_fresh_files():
    Image = _pillow()
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:37, 0:45]
    smooth = np.stack([(x * 5 + y) & 255, (x + y * 3) & 255, (x * y) & 255], -1).astype(np.uint8)
    noise = rng.integers(0, 256, (37, 45, 3), dtype=np.uint8)
    mix = np.where(((x // 8 + y // 8) & 1)[..., None] == 1, smooth, noise).astype(np.uint8)
    for name, arr in (("smooth", smooth), ("noise", noise), ("mix", mix)):
        for q, m in ((5, 0), (60, 4), (95, 6)):
            b = io.BytesIO()
            Image.fromarray(arr).save(b, "WEBP", quality=q, method=m)
            d = b.getvalue()
            bgr, _, st = R.decode_stages(d)
            want = np.asarray(Image.open(io.BytesIO(d)).convert("RGBA"))[..., 2::-1]
            assert st == 0 and np.array_equal(bgr, want), (name, q, m)
            assert WL.supported(d) and not W.supported(d)


def test_rule_book_predicts_the_malformed_status(cases):
    want = {"cut_one_more": WL.STATUS_INPUT_EXHAUSTED, "token_partition_half": WL.STATUS_INPUT_EXHAUSTED, "first_partition_half": None,
            "partition_size_past_chunk": WL.STATUS_BAD_PARTITIONS, "partition_table_past_chunk": WL.STATUS_BAD_PARTITIONS}
    assert sorted(_names(cases, "bad_names")) == sorted(want)
    for n, w in want.items():
        d = cases["badfile_" + n].tobytes()
        assert WL.supported(d), n                                     # the container and the 10 header bytes are intact: only the decoder can tell
        bgr, _, st = R.decode_stages(d)
        assert st == int(cases["badstatus_" + n]) and st != 0 and not bgr.any(), n
        assert w is None and st & WL.STATUS_INPUT_EXHAUSTED or st == w, n
    assert (WL.STATUS_INPUT_EXHAUSTED, WL.STATUS_BAD_PARTITIONS) == (R.STATUS_INPUT_EXHAUSTED, R.STATUS_BAD_PARTITIONS) == (1, 2)
    assert WL.status_text(3) == "a partition that ends early, partition sizes that run past the chunk or leave the last partition empty"
    # the lazy reader: the file with the largest cut that still decodes is a GOOD case, one byte more is not
    ok = [n for n in _names(cases) if n.startswith("cut_")]
    assert len(ok) == 1 and int(ok[0].split("_")[1]) >= 1


def test_transcode_and_the_bool_writer(cases):
    d = _file(cases, "mixed_17x33_q75_m4")
    a, b = R.decode_stages(d), R.decode_stages(R.transcode(d))
    assert a[2] == b[2] == 0 and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])) and np.array_equal(a[0], b[0])
    eight = R.transcode(d, log2_parts=3, simple=1, colorspace=1)
    f, st, parts = R.describe(eight)
    assert st == 0 and len(parts) == 9 and f.simple == 1 and f.colorspace == 1 and WL.supported(eight)
    rng = np.random.default_rng(3)
    bits, probs = rng.integers(0, 2, 4000), rng.integers(1, 256, 4000)
    enc = R.BoolEncoder()
    for bit, p in zip(bits, probs):
        enc.bit(int(p), int(bit))
    buf = enc.finish()
    dec = R.BoolDecoder(buf, 0, len(buf))
    assert [dec.bit(int(p)) for p in probs] == [int(v) for v in bits] and not dec.eof


def test_the_two_copies_of_the_tables_agree():
    with open(os.path.join(ROOT, "maf-yolo_amd", "csrc", "vp8_tables.h")) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    got = {name: [int(v) for v in re.findall(r"\d+", body)] for name, body in re.findall(r"(k_vp8_\w+)(?:\[\d+\])+\s*=\s*\{(.*?)\};", text, flags=re.S)}
    assert got["k_vp8_coeff_proba0"] == T.COEFF_PROBA0.reshape(-1).tolist() and got["k_vp8_coeff_update"] == T.COEFF_UPDATE.reshape(-1).tolist()
    assert got["k_vp8_bmode_proba"] == T.BMODE_PROBA.reshape(-1).tolist()
    assert got["k_vp8_dc_q"] == T.DC_Q.tolist() and got["k_vp8_ac_q"] == T.AC_Q.tolist()
    assert got["k_vp8_zigzag"] == list(T.ZIGZAG) and got["k_vp8_bands"] == list(T.BANDS)
    assert [v for v in got["k_vp8_cat3456"] if v] == [v for c in T.CAT3456 for v in c]


def test_parse_reads_every_case(cases):
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        s, e = R.vp8_payload(d)
        f, st, parts = R.describe(d)
        info = WL.parse(d)
        assert (info.width, info.height) == (f.width, f.height) and info.stream == (s + 10, e), n
        assert info.first_partition == parts[0][1] - parts[0][0] and info.profile <= 3, n
        assert info.extended == (n.startswith("rgba") or n.startswith("iccp")) and info.has_alpha == n.startswith("rgba"), n
        assert info.orientation == (1 if n.startswith("iccp") else None), n
    scaled = WL.parse(_file(cases, "t_ignored_bits"))
    assert (scaled.width, scaled.height) == (50, 40)                   # the scale hints above the 14 size bits are ignored


def _exif(orientation, prefix):
    tiff = b"II*\x00\x08\x00\x00\x00\x01\x00" + struct.pack("<HHIHH", 0x0112, 3, 1, orientation, 0) + b"\x00\x00\x00\x00"
    return (b"Exif\x00\x00" if prefix else b"") + tiff


def test_unsupported_kinds_are_named(cases, monkeypatch, golden):
    pay = _payload(cases)
    vp8 = _chunk(b"VP8 ", pay)

    def raises(d, word):
        with pytest.raises(W.WebpUnsupported, match=word):
            WL.parse(d)
        assert not WL.supported(d)

    raises(_riff(_vp8x(33, 17, 0x02), vp8), "animation flag")
    raises(_riff(_vp8x(33, 17), _chunk(b"ANIM", bytes(6)), vp8), "ANIM chunk")
    raises(_riff(_vp8x(33, 17), _chunk(b"ANMF", bytes(16)), vp8), "ANMF chunk")
    lossless = golden("webp_cases")
    raises(lossless["file_" + str(lossless["names"][0])].tobytes(), "lossless file .* webp.decode takes it")
    monkeypatch.setattr(WL.staging, "MAX_BLOB", 3 * 33 * 17)
    raises(_riff(vp8), "33 x 17 .* is beyond")
    monkeypatch.undo()
    for prefix in (True, False):
        d = _riff(_vp8x(33, 17, 0x08), vp8, _chunk(b"EXIF", _exif(6, prefix)))
        assert WL.parse(d).orientation == 6 and not WL.supported(d) and WL.supported(d, ignore_orientation=True)
        with pytest.raises(W.WebpUnsupported, match=r"file 0: webp_lossy: an EXIF orientation of 6"):
            WL.decode([d], device="cuda:0")
    # skipped: alpha (dropped), ICCP, XMP, unknown chunks
    d = _riff(_vp8x(33, 17, 0x10), _chunk(b"ICCP", b"abc"), _chunk(b"ALPH", b"\x00\x01\x02"), vp8, _chunk(b"XMP ", b"<x/>"), _chunk(b"what", b"?"))
    info = WL.parse(d)
    assert WL.supported(d) and info.has_alpha and info.extended and d[info.stream[0]:info.stream[1]] == pay[10:]


def test_corrupt_files_raise_maferror(cases):
    pay = _payload(cases)
    good = _riff(_chunk(b"VP8 ", pay))
    assert WL.supported(good)

    def raises(d, word):
        with pytest.raises(MafError, match=word) as e:
            WL.parse(d)
        assert not isinstance(e.value, W.WebpUnsupported)
        assert not WL.supported(d)

    def patched(at, value):
        return _riff(_chunk(b"VP8 ", pay[:at] + bytes(value) + pay[at + len(value):]))

    raises(b"", "signature")
    raises(good[:-3], "RIFF size runs past")
    raises(_riff(_chunk(b"ICCP", b"abcd")), "no image chunk")
    raises(_riff(_chunk(b"VP8 ", pay[:9])), "shorter than its 10 header bytes")
    raises(patched(0, [pay[0] | 1]), "not a key frame")
    raises(patched(0, [pay[0] | 0x0e]), "profile 7")
    raises(patched(0, [pay[0] & ~0x10]), "invisible")
    raises(patched(3, [0x9d, 0x01, 0x2b]), "start code")
    raises(patched(6, [0, 0xc0]), "a frame of 0 x 17")
    raises(patched(8, [0, 0]), "a frame of 33 x 0")
    raises(patched(0, [pay[0] | 0xe0, 0xff, 0xff]), "first partition .* runs past")
    raises(_riff(_vp8x(34, 17), _chunk(b"VP8 ", pay)), "canvas 34 x 17 disagrees with the VP8 size 33 x 17")
    raises(_riff(_chunk(b"VP8 ", pay), _vp8x(33, 17)), "misplaced or malformed VP8X")


def test_decode_names_the_file(cases, tmp_path, golden):
    lossless = golden("webp_cases")
    p = tmp_path / "lossless.webp"
    p.write_bytes(lossless["file_" + str(lossless["names"][0])].tobytes())
    # the files are parsed before the device is touched
    with pytest.raises(W.WebpUnsupported, match=r"file 1 \(.*lossless\.webp\): webp_lossy: a lossless file"):
        WL.decode([_file(cases), str(p)], device="cuda:0")
    with pytest.raises(MafError, match=r"file 0: webp: no RIFF / WEBP signature"):
        WL.decode([b"GIF89a" + bytes(20)], device="cuda:0")
    with pytest.raises(MafError, match="no files"):
        WL.decode([], device="cuda:0")


def test_blob_layout_and_struct_sizes(cases):
    pick = ["mixed_64x65_q75_m4", "flat_1x1_q30_m0", "rgba_33x17_q75_m4"]
    datas = [cases["file_" + n].tobytes() for n in pick]
    infos = [WL.parse(d) for d in datas]
    hdr, images = WL.build_blob(infos)
    buf = np.full(int(hdr["total_bytes"]), 0xAA, np.uint8)
    WL.fill_blob(buf, hdr, images, datas, infos)
    so = int(hdr["stream_off"])
    scr = pl = 0
    for d, im, info in zip(datas, images, infos):
        s, e = R.vp8_payload(d)
        assert buf[so + int(im["stream_begin"]):so + int(im["stream_end"])].tobytes() == d[s + 10:e]        # the container and the 10 header bytes are gone
        mbw, mbh = WL.macroblocks(info.width, info.height)
        assert (mbw, mbh) == ((info.width + 15) // 16, (info.height + 15) // 16)
        assert int(im["scratch_off"]) == scr and int(im["scratch_bytes"]) == WL.scratch_bytes(info.width, info.height) == 256 + mbw * mbh * 800
        assert int(im["planes_off"]) == pl and pl % 16 == 0 and scr % 16 == 0 and int(im["out_off"]) % 16 == 0
        assert (int(im["w"]), int(im["h"]), int(im["first_part_bytes"])) == (info.width, info.height, info.first_partition)
        scr += int(im["scratch_bytes"])
        pl += 384 * mbw * mbh
    assert int(hdr["scratch_bytes"]) == scr and int(hdr["plane_bytes"]) == pl and int(hdr["out_bytes"]) >= sum(3 * i.width * i.height for i in infos)
    end = so + int(images[-1]["stream_end"])
    assert int(hdr["total_bytes"]) - end >= WL.STREAM_PAD and not buf[end:].any()
    assert int(hdr["images_off"]) % 16 == 0 and so % 16 == 0
    assert (WL.HEADER_DT.itemsize, WL.IMAGE_DT.itemsize) == (64, 64)
    L = lib.load()                                                    # the built library: a missing one raises
    WL._bind(L)
    sizes = (ctypes.c_int32 * 2)()
    lib.check(L.maf_vp8_struct_sizes(sizes))
    assert list(sizes) == [WL.HEADER_DT.itemsize, WL.IMAGE_DT.itemsize]


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
            if name == "maf_vp8_struct_sizes" and typ == "int32_t*":
                args.append(_CTYPES[typ])
            elif typ.endswith("*") or typ == "maf_vp8_stream_t":
                args.append(ctypes.c_void_p)
            else:
                args.append(_CTYPES[typ])
        out[name] = (_CTYPES[ret], args)
    return out


def test_binding_equals_the_header():
    with open(os.path.join(ROOT, "include", "mafyolo_vp8.h")) as f:
        text = f.read()
    protos = _header_prototypes(text)
    assert sorted(protos) == ["maf_vp8_decode", "maf_vp8_struct_sizes"] == sorted(WL.PROTOTYPES)
    for name, (res, args) in protos.items():
        assert WL.PROTOTYPES[name] == (res, args), name
    assert len(protos["maf_vp8_decode"][1]) == 9
    L = WL._bind(lib.load())
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the constants the binding repeats
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(MAF_VP8_\w+)\s+(\d+)\b", text)}
    assert [defs["MAF_VP8_ST_" + n] for n in ("INPUT_EXHAUSTED", "BAD_PARTITIONS")] == [b for b, _ in WL._STATUS_TEXT]
    assert (defs["MAF_VP8_STREAM_PAD"], defs["MAF_VP8_MAX_SIDE"], defs["MAF_VP8_STAGE_ALL"]) == (WL.STREAM_PAD, WL.MAX_SIDE, WL.STAGE_ALL)
    assert [defs["MAF_VP8_STAGE_" + n] for n in ("PARSE", "RECON", "FILTER", "CONVERT")] == [WL.STAGE_PARSE, WL.STAGE_RECON, WL.STAGE_FILTER, WL.STAGE_CONVERT]
    assert (defs["MAF_VP8_META_WORDS"], defs["MAF_VP8_MB_RECORD"], defs["MAF_VP8_MB_COEFFS"]) == (WL.META_WORDS, WL.MB_RECORD, WL.MB_COEFFS)
    # outside the signature table and outside the lossless header, whose two functions stay two
    for other in ("mafyolo_hip.h", "mafyolo_webp.h"):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert "maf_vp8" not in f.read(), other
    assert not [n for n in lib.EXPORTS if "vp8" in n] and not [n for n in lib.TYPED_POINTERS if "vp8" in n]
    assert sorted(W.PROTOTYPES) == ["maf_webp_decode", "maf_webp_struct_sizes"]


def test_router_without_the_flag_refuses_lossy_files_as_before(cases):
    d = _file(cases)
    assert F.kind(d) is None and F.kind(d, webp=True) == "webp" and F.kind(d, lossy=True) is None and F.kind(d, webp=True, lossy=True) == "webp_lossy"
    lossless = _riff(_chunk(b"VP8L", b"\x2f" + bytes(8)))
    assert F.kind(lossless, webp=True, lossy=True) == "webp" and F.kind(_riff(_vp8x(3, 2), _chunk(b"ALPH", b"ab"), _chunk(b"VP8 ", bytes(12))), True, True) == "webp_lossy"
    assert F.kind(b"RIFF\x00\x00\x00\x00WEBP", webp=True, lossy=True) == "webp"          # no image chunk: webp.decode names what is wrong
    assert F.kind(P.SIGNATURE + bytes(8), webp=True, lossy=True) == "png" and F.kind(b"\xff\xd8\xff", webp=True, lossy=True) == "jpeg"
    with pytest.raises(MafError, match="file 0: neither a JPEG nor a PNG signature"):
        F.decode([d], device="cuda:0")
    with pytest.raises(MafError, match="file 0: neither a JPEG nor a PNG signature"):
        F.decode([d], device="cuda:0", lossy=True)                      # lossy=True alone asks for nothing
    with pytest.raises(W.WebpUnsupported, match=r"file 0: webp: a lossy file \(a 'VP8 ' chunk\) is not supported \(lossless VP8L only\) \[webp files of this call are inputs \[0\]\]"):
        F.decode([d], device="cuda:0", webp=True)
    with pytest.raises(W.WebpUnsupported, match=r"a lossy file"):
        W.parse(d)
    assert not W.supported(d)


def test_router_sniffs_and_keeps_the_order(monkeypatch, cases, golden):
    lossy_file = _file(cases)
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
        assert all(F.kind(f, webp=True) == "webp" for f in files)
        return ["w%d" % i for i in range(len(files))]

    def fake_lossy(files, device=None, stream=None, check=True, ignore_orientation=False):
        calls.append(("webp_lossy", len(files), ignore_orientation, device, stream))
        assert all(F.kind(f, webp=True, lossy=True) == "webp_lossy" for f in files)
        return ["l%d" % i for i in range(len(files))]

    monkeypatch.setattr(J, "decode", fake_jpeg)
    monkeypatch.setattr(P, "decode", fake_png)
    monkeypatch.setattr(W, "decode", fake_webp)
    monkeypatch.setattr(WL, "decode", fake_lossy)
    got = F.decode([lossy_file, webp_file, png_file, jpeg_file, lossy_file, jpeg_file, png_file, webp_file, lossy_file], device="cuda:0", stream="s",
                   progressive=True, ignore_orientation=True, webp=True, lossy=True)
    assert got == ["l0", "w0", "p0", "j0", "l1", "j1", "p1", "w1", "l2"] and F.kind(webp_file, webp=True, lossy=True) == "webp"
    assert sorted(calls) == [("jpeg", 2, True, True, "cuda:0", "s"), ("png", 2, "cuda:0", "s"), ("webp", 2, True, "cuda:0", "s"),
                             ("webp_lossy", 3, True, "cuda:0", "s")]
    calls.clear()
    assert F.decode([lossy_file], webp=True, lossy=True) == ["l0"] and calls == [("webp_lossy", 1, False, None, None)]
    calls.clear()
    # without lossy=True the lossy file goes where it went before: to webp.decode, which refuses it
    assert F.decode([lossy_file, webp_file], webp=True) == ["w0", "w1"] and calls == [("webp", 2, False, None, None)]
