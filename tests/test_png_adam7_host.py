"""No GPU: Adam7 PNG on the host: the rule book (tests/png_adam7_ref.py), png.parse(..., interlaced=True), the blob, the router's new flags.

* the rule book equals the fixtures (tests/golden/png_adam7_cases.npz, written by tools/make_golden_png_adam7.py: Pillow's pixels), zlib.decompress
  and a fresh Pillow decode on every case, and predicts the stored status word of every malformed file;
* parse(..., interlaced=True) gives the pass-sum sizes (1 x 1: the one byte pair of pass 1; below 8 bits the rows can exceed h * rowbytes);
  without the flag an Adam7 file is refused as before; interlace method 2 is refused with the flag too; the 2 GiB limit applies to the pass sum;
* the blob carries the flag in the renamed field of an image table whose size is still 80 bytes, and its rows buffer is sized by the pass sums;
* frames.decode hands interlaced / apply_orientation on only when they are set (the decoders mocked with and without the new keywords).
"""
import io
import zlib

import numpy as np
import pytest

import png_adam7_ref as A
import png_ref as R
from maf_yolo_amd import frames as F, jpeg as J, png as P


@pytest.fixture(scope="module")
def cases(golden):
    return golden("png_adam7_cases")


def _names(z):
    return [str(n) for n in z["names"]]


def test_rule_book_equals_the_fixtures_zlib_and_a_fresh_pillow_decode(cases):
    from PIL import Image                                             # the judge: its absence is a failure, not a skip
    names = _names(cases)
    assert len(names) == 37
    for n in names:
        d = cases["file_" + n].tobytes()
        bgr, inflated, flat, st = A.decode_stages(d)
        assert st == 0, n
        assert bgr.dtype == np.uint8 and np.array_equal(bgr, cases["bgr_" + n]), n
        assert np.array_equal(inflated, cases["inflated_" + n]) and inflated.tobytes() == zlib.decompress(R.walk(d)[2]), n
        im = Image.open(io.BytesIO(d))
        assert im.info.get("interlace") == 1, n
        if im.mode.startswith("I"):
            want = np.repeat((np.asarray(im).astype(np.int64) >> 8).astype(np.uint8)[:, :, None], 3, 2)
        else:
            im.info.pop("transparency", None)
            want = np.asarray(im.convert("RGBA" if im.mode in ("LA", "RGBA") else "RGB"))[:, :, 2::-1]
        assert np.array_equal(cases["bgr_" + n], want), n


def test_rule_book_predicts_the_malformed_status(cases):
    want = {"filter_byte_7_in_pass3": P.STATUS_BAD_FILTER, "idat_cut_to_half": P.STATUS_INPUT_EXHAUSTED,
            "plain_stream_under_interlaced_header": P.STATUS_TOO_FEW_BYTES | P.STATUS_BAD_FILTER,
            "palette_index_past_plte_in_pass7": P.STATUS_BAD_PALETTE_INDEX}
    assert sorted(str(n) for n in cases["bad_names"]) == sorted(want)
    for n, w in want.items():
        d = cases["badfile_" + n].tobytes()
        assert P.supported(d, interlaced=True) and not P.supported(d), n      # the chunks are intact: only the decoder can tell
        inflated, st = A.decode_stages(d)[1::2]
        assert st == w == int(cases["badstatus_" + n]), n
        assert inflated.size == P.parse(d, interlaced=True).inflated_size, n


def test_parse_gives_the_pass_sums(cases):
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        (w, h, depth, ctype, _, _, lace), plte, z = R.walk(d)
        with pytest.raises(P.PngUnsupported, match="Adam7"):
            P.parse(d)
        info = P.parse(d, interlaced=True)
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (w, h, depth, ctype, 1) and lace == 1, n
        bits = R.CHANNELS[ctype] * depth
        assert info.rowbytes == (w * bits + 7) // 8 and info.bpp == max(1, bits // 8), n
        assert (info.inflated_size, P.rows_size(info)) == A.sizes(w, h, bits), n
        assert info.inflated_size == cases["inflated_" + n].size, n
    # the sums by hand: 1 x 1 is one filter byte and one row byte of pass 1; 8 x 8 RGB 8 has the passes 1x1 1x1 2x1 2x2 4x2 4x4 8x4
    assert A.sizes(1, 1, 24) == (4, 3) and A.sizes(1, 1, 1) == (2, 1)
    assert A.sizes(8, 8, 24) == (1 * 4 + 1 * 4 + 1 * 7 + 2 * 7 + 2 * 13 + 4 * 13 + 4 * 25, 64 * 3)
    assert [g[4:] for g in A.geometry(17, 33, 1)][0] == (3, 5, 1)     # 17 wide at depth 1: pass 1 has 3 pixels, a row that ends mid-byte
    assert [g[4:6] for g in A.geometry(37, 131, 8)][6] == (37, 65)    # pass 7 has 65 rows: one past a 64-row band
    assert [g[4:6] for g in A.geometry(1, 9, 8)] == [(1, 2), (0, 2), (1, 1), (0, 3), (1, 2), (0, 5), (1, 4)]
    assert P.adam7_passes(1, 9, 8) == [g[4:] for g in A.geometry(1, 9, 8)]
    g1 = P.parse(cases["file_gray1_17x33"].tobytes(), interlaced=True)
    assert P.rows_size(g1) > g1.height * g1.rowbytes                  # sub-byte rows pad once per pass row
    plain = P.parse(R.encode(np.zeros((3, 3), np.uint8), 3, 8, 0)[0], interlaced=True)
    assert plain.interlace == 0 and plain.inflated_size == 3 * 4 and P.rows_size(plain) == 9
    assert P.PngInfo(1, 1, 8, 0, None, (), 2, 1, 1, 1).interlace == 0     # the new field is trailing and defaulted


def test_refusals():
    z = zlib.compress(bytes(64))
    two = R.assemble(17, 33, 8, 2, z, interlace=2)
    for flag in (False, True):
        with pytest.raises(P.PngUnsupported, match="interlace method 2"):
            P.parse(two, interlaced=flag)
        assert not P.supported(two, interlaced=flag)
    big = R.assemble(65535, 65535, 16, 6, z, interlace=1)
    with pytest.raises(P.PngUnsupported, match="2 GiB"):
        P.parse(big, interlaced=True)
    with pytest.raises(P.PngUnsupported, match=r"^file 1: png: Adam7"):
        P.decode([R.assemble(1, 1, 8, 0, z), R.assemble(1, 1, 8, 0, z, interlace=1)], device="cuda:0")      # parsed before the device is touched


def test_blob_carries_the_flag_in_a_table_of_the_same_size(cases, golden):
    plain = golden("png_cases")["file_gray1_17x33"].tobytes()
    datas = [cases["file_gray1_17x33"].tobytes(), plain, cases["file_pal4_8x8"].tobytes()]
    infos = [P.parse(d, interlaced=True) for d in datas]
    hdr, images, palette = P.build_blob(infos)
    assert (P.HEADER_DT.itemsize, P.IMAGE_DT.itemsize) == (72, 80) and P.IMAGE_DT.names[-1] == "interlace"
    assert P.IMAGE_DT.fields["interlace"][1] == 76 and "reserved" not in P.IMAGE_DT.names
    assert images["interlace"].tolist() == [1, 0, 1]
    assert images["inflated_size"].tolist() == [A.sizes(17, 33, 1)[0], 33 * 4, A.sizes(8, 8, 4)[0]]
    want_rows = [A.sizes(17, 33, 1)[1], 33 * 3, A.sizes(8, 8, 4)[1]]
    assert images["rows_off"].tolist() == [0, P._align(want_rows[0]), P._align(want_rows[0]) + P._align(want_rows[1])]
    assert int(hdr["rows_bytes"]) == sum(P._align(r) for r in want_rows)
    buf = np.zeros(int(hdr["total_bytes"]), np.uint8)
    P.fill_blob(buf, hdr, images, palette, datas, infos)
    table = np.frombuffer(buf[int(hdr["images_off"]):int(hdr["images_off"]) + 3 * 80].tobytes(), P.IMAGE_DT)
    assert table["interlace"].tolist() == [1, 0, 1]
    # a plain file's record is what it was: the field that was `reserved` stays 0
    alone = P.build_blob([P.parse(plain)])[1][0]
    assert int(alone["interlace"]) == 0


def test_router_hands_the_new_flags_on_only_when_set(monkeypatch, golden, cases):
    png_file = cases["file_rgb8_1x1"].tobytes()
    jz = golden("jpeg_cases")
    jpeg_file = jz["file_" + str(jz["names"][0])].tobytes()
    calls = []

    def old_jpeg(files, device=None, stream=None, ignore_orientation=False, check=True, progressive=False):
        calls.append(("jpeg", len(files)))
        return ["j"] * len(files)

    def old_png(files, device=None, stream=None, check=True):
        calls.append(("png", len(files)))
        return ["p"] * len(files)

    def new_jpeg(files, device=None, stream=None, ignore_orientation=False, check=True, progressive=False, apply_orientation=False):
        calls.append(("jpeg", len(files), apply_orientation))
        return ["j"] * len(files)

    def new_png(files, device=None, stream=None, check=True, interlaced=False):
        calls.append(("png", len(files), interlaced))
        return ["p"] * len(files)

    mix = [png_file, jpeg_file, png_file]
    monkeypatch.setattr(J, "decode", old_jpeg)
    monkeypatch.setattr(P, "decode", old_png)
    assert F.decode(mix) == ["p", "j", "p"] and sorted(calls) == [("jpeg", 1), ("png", 2)]      # unset: the decoders never see the keywords
    with pytest.raises(TypeError, match="interlaced"):
        F.decode(mix, interlaced=True)
    with pytest.raises(TypeError, match="apply_orientation"):
        F.decode([jpeg_file], apply_orientation=True)
    calls.clear()
    monkeypatch.setattr(J, "decode", new_jpeg)
    monkeypatch.setattr(P, "decode", new_png)
    assert F.decode(mix, interlaced=True) == ["p", "j", "p"] and sorted(calls) == [("jpeg", 1, False), ("png", 2, True)]
    calls.clear()
    assert F.decode(mix, apply_orientation=True) == ["p", "j", "p"] and sorted(calls) == [("jpeg", 1, True), ("png", 2, False)]
