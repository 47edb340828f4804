"""No GPU: the RIFF walk (maf-yolo_amd/webp.py parse), the rule book (tests/webp_ref.py), the hand-written binding and the router.

* webp_ref equals the fixtures (tests/golden/webp_cases.npz, written by tools/make_golden_webp.py: Pillow's pixels) and, where Pillow has
  libwebp, a fresh Pillow decode of every fixture and of files written here (four contents x methods 0 / 4 / 6);
* it predicts the stored status word of every malformed fixture;
* parse classifies every refusal with its exception class and message, and decode names the offending file before the device is touched;
* blob layout and alignment; the struct sizes equal maf_webp_struct_sizes of the built library;
* the prototypes of include/mafyolo_webp.h, read by regex, equal webp.py's argtypes and restype; neither function is in lib.EXPORTS nor in
  mafyolo_hip.h;
* the router: without webp=True nothing changes, with it order and hand-on of the flags are right (the decoders replaced by fakes).
"""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

import webp_ref as R
from maf_yolo_amd import frames as F, jpeg as J, lib, png as P, webp as W
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
    return golden("webp_cases")


def _names(z, key="names"):
    return [str(n) for n in z[key]]


def _plain():
    return R.riff(R.hand_payload(3, 2))


def test_rule_book_equals_the_fixtures(cases):
    assert len(_names(cases)) >= 25
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        bgr, argb, st = R.decode_stages(d)
        assert st == 0, n
        assert bgr.dtype == np.uint8 and np.array_equal(bgr, cases["bgr_" + n]), n
        assert argb.dtype == np.uint32 and np.array_equal(argb, cases["argb_" + n]), n
        info = W.parse(d)
        assert (info.height, info.width, 3) == bgr.shape and argb.shape[0] == info.height and argb.shape[1] <= info.width, n


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
    rgba = np.concatenate([smooth, noise[..., :1]], -1)
    for name, arr, mode in (("smooth", smooth, "RGB"), ("noise", noise, "RGB"), ("mix", mix, "RGB"), ("rgba", rgba, "RGBA")):
        for m in (0, 4, 6):
            b = io.BytesIO()
            Image.fromarray(arr, mode).save(b, "WEBP", lossless=True, method=m, exact=True)
            d = b.getvalue()
            bgr, _, st = R.decode_stages(d)
            want = np.asarray(Image.open(io.BytesIO(d)).convert("RGBA"))[..., 2::-1]
            assert st == 0 and np.array_equal(bgr, want) and np.array_equal(bgr, arr[..., 2::-1]), (name, m)
            assert W.supported(d)


def test_rule_book_predicts_the_malformed_status(cases):
    want = {"stream_cut_to_half": W.STATUS_INPUT_EXHAUSTED, "oversubscribed_code": W.STATUS_BAD_CODE_LENGTHS, "incomplete_code": W.STATUS_BAD_CODE_LENGTHS,
            "max_symbol_above_alphabet": W.STATUS_BAD_CODE_LENGTHS, "zero_run_past_alphabet": W.STATUS_BAD_CODE_LENGTHS, "cache_bits_0": W.STATUS_BAD_CACHE_BITS,
            "cache_bits_12": W.STATUS_BAD_CACHE_BITS, "transform_twice": W.STATUS_BAD_TRANSFORM, "distance_beyond_produced": W.STATUS_DISTANCE_TOO_FAR,
            "copy_past_last_pixel": W.STATUS_COPY_PAST_END}
    assert sorted(_names(cases, "bad_names")) == sorted(want)
    for n, w in want.items():
        d = cases["badfile_" + n].tobytes()
        assert W.supported(d), n                                      # the container is intact: only the decoder can tell
        bgr, _, st = R.decode_stages(d)
        assert st == w == int(cases["badstatus_" + n]) and not bgr.any(), n
    assert (W.STATUS_INPUT_EXHAUSTED, W.STATUS_TABLE_SPACE) == (R.ST_INPUT_EXHAUSTED, R.ST_TABLE_SPACE) == (1, 128)
    assert W.status_text(W.STATUS_COPY_PAST_END | W.STATUS_INPUT_EXHAUSTED) == "a bit stream that ends early, a copy that runs past the last pixel"


def test_parse_reads_every_case(cases):
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        pay, w, h = R.walk(d)
        info = W.parse(d)
        assert (info.width, info.height) == (w, h) and d[info.stream[0]:info.stream[1]] == pay[5:], n
        assert info.extended == n.startswith("vp8x") and info.orientation is None, n
    assert W.parse(cases["file_rgba_m4_17x33"].tobytes()).has_alpha_hint
    assert not W.parse(cases["file_mix_m4_17x33"].tobytes()).has_alpha_hint


def _exif(orientation, prefix):
    tiff = b"II*\x00\x08\x00\x00\x00\x01\x00" + struct.pack("<HHIHH", 0x0112, 3, 1, orientation, 0) + b"\x00\x00\x00\x00"
    return (b"Exif\x00\x00" if prefix else b"") + tiff


def test_unsupported_kinds_are_named(monkeypatch):
    pay = R.hand_payload(3, 2)

    def raises(d, word):
        with pytest.raises(W.WebpUnsupported, match=word):
            W.parse(d)
        assert not W.supported(d)

    raises(b"RIFF" + struct.pack("<I", 4 + 8 + 10) + b"WEBP" + R.chunk(b"VP8 ", bytes(10)), "lossy")
    raises(R.riff(pay, extended=(3, 2, 0x10), before=((b"ALPH", b"\x00\x01"),)), "lossy")
    raises(R.riff(pay, extended=(3, 2, 0x02)), "animation flag")
    raises(R.riff(pay, extended=(3, 2), before=((b"ANIM", bytes(6)),)), "ANIM chunk")
    raises(R.riff(pay, extended=(3, 2), before=((b"ANMF", bytes(16)),)), "ANMF chunk")
    raises(R.riff(R.hand_payload(3, 2, version=1)), "version 1")
    monkeypatch.setattr(W.staging, "MAX_BLOB", 3 * 3 * 2)               # the 14-bit size fields keep 3 * w * h below the real limit
    raises(R.riff(pay), "3 x 2 .* is beyond")
    monkeypatch.undo()
    # an EXIF orientation: parse reads it, decode refuses it unless told to ignore it
    for prefix in (True, False):
        d = R.riff(pay, extended=(3, 2, 0x08), after=((b"EXIF", _exif(6, prefix)),))
        assert W.parse(d).orientation == 6 and not W.supported(d) and W.supported(d, ignore_orientation=True)
        with pytest.raises(W.WebpUnsupported, match=r"file 0: webp: an EXIF orientation of 6"):
            W.decode([d], device="cuda:0")
    d = R.riff(pay, extended=(3, 2, 0x08), after=((b"EXIF", _exif(1, True)),))
    assert W.parse(d).orientation == 1 and W.supported(d)
    assert W.supported(R.riff(pay)) and W.supported(R.riff(pay, extended=(3, 2), before=((b"XMP ", b"<x/>"), (b"ICCP", b"abc"))))


def test_corrupt_files_raise_maferror():
    pay = R.hand_payload(3, 2)
    good = R.riff(pay)

    def raises(d, word):
        with pytest.raises(MafError, match=word) as e:
            W.parse(d)
        assert not isinstance(e.value, W.WebpUnsupported)
        assert not W.supported(d)

    raises(b"", "signature")
    raises(P.SIGNATURE + good, "signature")
    raises(good[:-3], "RIFF size runs past")
    raises(good[:16] + struct.pack("<I", len(pay) + 40) + good[20:], "chunk 'VP8L' runs past")
    raises(R.riff(b"\x2e" + pay[1:]), "0x2f")
    raises(b"RIFF" + struct.pack("<I", 4) + b"WEBP", "no image chunk")
    body = R.chunk(b"VP8L", pay) + b"ABCD\x01"
    raises(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body, "chunk header runs past")
    raises(b"RIFF" + struct.pack("<I", 4 + 12) + b"WEBP" + R.chunk(b"ICCP", b"abcd"), "no image chunk")
    raises(R.riff(pay, extended=(4, 2)), "canvas 4 x 2 disagrees with the VP8L size 3 x 2")


def test_decode_names_the_file(tmp_path):
    p = tmp_path / "lossy.webp"
    p.write_bytes(b"RIFF" + struct.pack("<I", 4 + 8 + 10) + b"WEBP" + R.chunk(b"VP8 ", bytes(10)))
    # the files are parsed before the device is touched
    with pytest.raises(W.WebpUnsupported, match=r"file 1 \(.*lossy\.webp\): webp: a lossy file"):
        W.decode([_plain(), str(p)], device="cuda:0")
    with pytest.raises(MafError, match=r"file 0: webp: no RIFF / WEBP signature"):
        W.decode([b"GIF89a" + bytes(20)], device="cuda:0")


def test_blob_layout_and_struct_sizes(cases):
    pick = ["mix_m4_64x65", "hand_cache1_4x3", "vp8x_iccp_odd_17x33"]
    datas = [cases["file_" + n].tobytes() for n in pick]
    infos = [W.parse(d) for d in datas]
    hdr, images = W.build_blob(infos)
    buf = np.full(int(hdr["total_bytes"]), 0xAA, np.uint8)
    W.fill_blob(buf, hdr, images, datas, infos)
    so = int(hdr["stream_off"])
    scr = 0
    for d, im, info in zip(datas, images, infos):
        pay = R.walk(d)[0]
        assert buf[so + int(im["stream_begin"]):so + int(im["stream_end"])].tobytes() == pay[5:]        # the container and the 5 header bytes are gone
        nbytes = len(pay) - 5
        assert (int(im["dir_words"]), int(im["arena_units"])) == W.table_space(nbytes) == (2 * nbytes + 40, 64 * nbytes + 64)
        assert int(im["scratch_off"]) == scr and int(im["scratch_off"]) % 16 == 0 and int(im["scratch_bytes"]) % 16 == 0
        assert int(im["scratch_bytes"]) == W.scratch_bytes(info.width, info.height, *W.table_space(nbytes))
        assert int(im["argb_off"]) % 4 == 0 and int(im["out_off"]) % 16 == 0 and (int(im["w"]), int(im["h"])) == (info.width, info.height)
        scr += int(im["scratch_bytes"])
    assert int(hdr["scratch_bytes"]) == scr and int(hdr["argb_words"]) >= sum(i.width * i.height for i in infos)
    end = so + int(images[-1]["stream_end"])
    assert int(hdr["total_bytes"]) - end >= W.STREAM_PAD and not buf[end:].any() and int(hdr["stream_bytes"]) % 8 == 0
    assert int(hdr["images_off"]) % 16 == 0 and so % 16 == 0
    assert (W.HEADER_DT.itemsize, W.IMAGE_DT.itemsize) == (64, 64)
    L = lib.load()                                                    # the built library: a missing one raises
    W._bind(L)
    sizes = (ctypes.c_int32 * 2)()
    lib.check(L.maf_webp_struct_sizes(sizes))
    assert list(sizes) == [W.HEADER_DT.itemsize, W.IMAGE_DT.itemsize]


_CTYPES = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int32_t*": ctypes.POINTER(ctypes.c_int32)}


def _header_prototypes(text):
    """name -> (restype, argtypes) of every function prototype of a C header: a scalar by its type, int32_t* as it is (the binding
    type-checks it), every other pointer (and the stream handle) as void*."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^\s*(int|void)\s+(maf_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        args = []
        for p in params.split(","):
            words = p.replace("*", " * ").split()
            typ = " ".join(w for w in words[:-1] if w != "const").replace(" *", "*")
            if name == "maf_webp_struct_sizes" and typ == "int32_t*":
                args.append(_CTYPES[typ])
            elif typ.endswith("*") or typ == "maf_webp_stream_t":
                args.append(ctypes.c_void_p)
            else:
                args.append(_CTYPES[typ])
        out[name] = (_CTYPES[ret], args)
    return out


def test_binding_equals_the_header():
    with open(os.path.join(ROOT, "include", "mafyolo_webp.h")) as f:
        text = f.read()
    protos = _header_prototypes(text)
    assert sorted(protos) == ["maf_webp_decode", "maf_webp_struct_sizes"] == sorted(W.PROTOTYPES)
    for name, (res, args) in protos.items():
        assert W.PROTOTYPES[name] == (res, args), name
    assert len(protos["maf_webp_decode"][1]) == 8
    L = W._bind(lib.load())
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the constants the binding repeats
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(MAF_WEBP_\w+)\s+(\d+)\b", text)}
    assert [defs["MAF_WEBP_ST_" + n] for n in ("INPUT_EXHAUSTED", "BAD_TRANSFORM", "BAD_CACHE_BITS", "BAD_CODE_LENGTHS", "NO_CODE", "DISTANCE_TOO_FAR",
                                                "COPY_PAST_END", "TABLE_SPACE")] == [b for b, _ in W._STATUS_TEXT]
    assert (defs["MAF_WEBP_STREAM_PAD"], defs["MAF_WEBP_MAX_SIDE"], defs["MAF_WEBP_STAGE_ALL"]) == (W.STREAM_PAD, W.MAX_SIDE, W.STAGE_ALL)
    # outside the 116-function table
    with open(os.path.join(ROOT, "include", "mafyolo_hip.h")) as f:
        assert "maf_webp" not in f.read()
    assert not [n for n in lib.EXPORTS if "webp" in n] and not [n for n in lib.TYPED_POINTERS if "webp" in n]


def test_router_is_unchanged_without_the_flag(cases):
    d = cases["file_mix_m4_17x33"].tobytes()
    assert F.kind(d) is None and F.kind(d, webp=True) == "webp" and F.kind(d, webp=False) is None
    assert F.kind(P.SIGNATURE + bytes(8), webp=True) == "png" and F.kind(b"\xff\xd8\xff", webp=True) == "jpeg" and F.kind(b"RIFF\x00\x00\x00\x00WAVE", webp=True) is None
    with pytest.raises(MafError, match="file 0: neither a JPEG nor a PNG signature"):
        F.decode([d], device="cuda:0")
    with pytest.raises(MafError, match="file 1: neither a JPEG nor a PNG signature"):
        F.decode([d, b"GIF89a"], device="cuda:0", webp=True)


def test_router_sniffs_and_keeps_the_order(monkeypatch, cases, golden):
    webp_file = cases["file_mix_m4_17x33"].tobytes()
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

    monkeypatch.setattr(J, "decode", fake_jpeg)
    monkeypatch.setattr(P, "decode", fake_png)
    monkeypatch.setattr(W, "decode", fake_webp)
    got = F.decode([webp_file, png_file, jpeg_file, webp_file, jpeg_file, png_file, webp_file], device="cuda:0", stream="s", progressive=True,
                   ignore_orientation=True, webp=True)
    assert got == ["w0", "p0", "j0", "w1", "j1", "p1", "w2"]
    assert sorted(calls) == [("jpeg", 2, True, True, "cuda:0", "s"), ("png", 2, "cuda:0", "s"), ("webp", 3, True, "cuda:0", "s")]
    calls.clear()
    assert F.decode([webp_file], webp=True) == ["w0"] and calls == [("webp", 1, False, None, None)]
    calls.clear()
    assert F.decode([png_file, jpeg_file]) == ["p0", "j0"] and sorted(calls) == [("jpeg", 1, False, False, None, None), ("png", 1, None, None)]
