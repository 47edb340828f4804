"""No GPU: EXIF orientation on the host: the rule book (tests/jpeg_orientation_ref.py), jpeg.supported / decode's refusals, the blob.

* the rule book (libjpeg's pixels by jpeg_ref / jpeg_progressive_ref, then the table) equals every frame of
  tests/golden/jpeg_orientation_cases.npz (PIL.ImageOps.exif_transpose of Pillow's decode) and a fresh exif_transpose;
* supported(..., apply_orientation=True) takes orientations 1 to 8 and no other tag value; without the flag nothing changes;
* decode refuses a tag value outside 1 to 8 and both orientation flags together, before the device is touched;
* the blob carries the orientation in the renamed field only when asked to, and the image table keeps its 88 bytes.
"""
import ctypes
import io

import numpy as np
import pytest

import jpeg_orientation_ref as O
from maf_yolo_amd import jpeg as J, lib
from maf_yolo_amd.lib import MafError


@pytest.fixture(scope="module")
def cases(golden):
    return golden("jpeg_orientation_cases")


def _names(z):
    return [str(n) for n in z["names"]]


def test_rule_book_equals_the_fixtures_and_a_fresh_exif_transpose(cases):
    from PIL import Image, ImageOps                                    # the judge: its absence is a failure, not a skip
    names = _names(cases)
    assert len(names) == 51 and sorted(set(cases["meta"][:, 2].tolist())) == list(range(1, 9))
    for n, (h, w, o, prog) in zip(names, cases["meta"].tolist()):
        d = cases["file_" + n].tobytes()
        info = J.parse(d, progressive=True)
        assert (info.height, info.width, info.orientation, info.scans is not None) == (h, w, o, bool(prog)), n
        got, want = O.decode(d), cases["bgr_" + n]
        assert got.shape == want.shape == ((w, h, 3) if o >= 5 else (h, w, 3)), n
        assert np.array_equal(got, want), n
        fresh = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(d))).convert("RGB"))[..., ::-1]
        assert np.array_equal(want, fresh), n


def test_table_on_a_grid_whose_pixels_name_their_place():
    h, w = 2, 3
    src = np.zeros((h, w, 3), np.uint8)
    src[..., 0], src[..., 1] = np.mgrid[0:h, 0:w]                      # pixel = (y, x, 0)
    corner = {o: tuple(O.orient(src, o)[0, 0, :2].tolist()) for o in range(1, 9)}      # which stored pixel becomes the top-left one
    assert corner == {1: (0, 0), 2: (0, 2), 3: (1, 2), 4: (1, 0), 5: (0, 0), 6: (1, 0), 7: (1, 2), 8: (0, 2)}
    assert [O.orient(src, o).shape[:2] for o in range(1, 9)] == [(2, 3)] * 4 + [(3, 2)] * 4
    assert np.array_equal(O.orient(src, 6), np.rot90(src, -1)) and np.array_equal(O.orient(src, 8), np.rot90(src, 1))
    assert np.array_equal(O.orient(src, 3), np.rot90(src, 2)) and np.array_equal(O.orient(src, 5), src.transpose(1, 0, 2))


def test_supported_and_the_refusals(cases):
    for n, (h, w, o, prog) in zip(_names(cases), cases["meta"].tolist()):
        d = cases["file_" + n].tobytes()
        assert J.supported(d, bool(prog)) == (o == 1), n                # without the flag: as before
        assert J.supported(d, bool(prog), apply_orientation=True), n
        assert J.supported(d, apply_orientation=True) == (not prog), n   # a progressive file still needs progressive=True
    for k, tag in (("tag0_file", 0), ("tag9_file", 9)):
        d = cases[k].tobytes()
        assert J.parse(d).orientation == tag
        assert not J.supported(d) and not J.supported(d, apply_orientation=True)
        with pytest.raises(J.JpegUnsupported, match=r"^file 0: jpeg: EXIF orientation %d is not one of 1 to 8$" % tag):
            J.decode([d], device="cuda:0", apply_orientation=True)     # parsed before the device is touched
        with pytest.raises(J.JpegUnsupported, match="orientation %d" % tag):
            J.decode([d], device="cuda:0")
    d = cases["file_o6_s2_13x22"].tobytes()
    with pytest.raises(MafError, match="apply_orientation and ignore_orientation exclude each other") as e:
        J.decode([d], device="cuda:0", apply_orientation=True, ignore_orientation=True)
    assert not isinstance(e.value, J.JpegUnsupported)
    with pytest.raises(J.JpegUnsupported, match="orientation 6"):
        J.decode([d], device="cuda:0")
    with pytest.raises(J.JpegUnsupported, match="progressive"):
        J.decode([cases["file_o6_prog_s2_13x22"].tobytes()], device="cuda:0", apply_orientation=True)


def test_blob_carries_the_orientation_only_when_asked(cases):
    names = ["o1_s2_13x22", "o6_s2_13x22", "o3_gray_5x11", "o8_prog_s2_13x22"]
    datas = [cases["file_" + n].tobytes() for n in names]
    infos = [J.parse(d, progressive=True) for d in datas]
    assert J.IMAGE_DT.itemsize == 88 and J.IMAGE_DT.names[-2:] == ("orientation", "reserved")
    assert J.IMAGE_DT.fields["orientation"][1] == 80 and J.IMAGE_DT.fields["reserved"][1] == 84
    sizes = (ctypes.c_int32 * 3)()
    lib.check(lib.load().maf_jpeg_struct_sizes(sizes))                 # the built library: a missing one raises
    assert list(sizes) == [J.HEADER_DT.itemsize, J.IMAGE_DT.itemsize, J.LANE_DT.itemsize]
    plain = J.build_blob(datas, infos)
    turned = J.build_blob(datas, infos, apply_orientation=True)
    assert plain[1]["orientation"].tolist() == [0, 0, 0, 0] and turned[1]["orientation"].tolist() == [1, 6, 3, 8]
    assert not plain[1]["reserved"].any() and not turned[1]["reserved"].any()
    # nothing else moves: the stored h and w, the offsets and the output allocation of 3 * w * h bytes per file
    for f in J.IMAGE_DT.names:
        if f != "orientation":
            assert np.array_equal(plain[1][f], turned[1][f]), f
    assert plain[0] == turned[0] and int(turned[0]["out_bytes"]) == sum(J._align(3 * i.width * i.height) for i in infos)
    buf = np.zeros(int(turned[0]["total_bytes"]), np.uint8)
    J.fill_blob(buf, turned[0], turned[1], turned[2], turned[3], turned[4], datas, infos, turned[5], turned[6])
    o = int(turned[0]["images_off"])
    assert np.frombuffer(buf[o:o + 4 * 88].tobytes(), J.IMAGE_DT)["orientation"].tolist() == [1, 6, 3, 8]
