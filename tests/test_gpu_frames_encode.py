"""-m gpu: frames.encode, the router in front of the four device encoders: a mixed list of suffixes (upper case included) returns, in input
order, what jpeg_encode, png_encode, tiff_encode and bmp_encode return alone; per-format arguments reach their encoder; rectangles; a suffix
without a device encoder (.webp, .dng) raises by name before anything is launched."""
import numpy as np
import pytest
import torch

from tiff_encode_ref import make_frame
import maf_yolo_amd as M
from maf_yolo_amd import bmp_encode, frames as F, jpeg_encode, png_encode, tiff_encode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SUFFIXES = [".jpg", ".TIF", ".png", ".bmp", ".JPEG", ".tiff", ".Bmp", ".mpo", ".PNG", ".tif"]
ALONE = {"jpeg": jpeg_encode.encode, "png": png_encode.encode, "tiff": tiff_encode.encode, "bmp": bmp_encode.encode}


@pytest.fixture(scope="module")
def frames():
    sizes = [(16, 24), (9, 7), (33, 47), (5, 3), (8, 8), (40, 31), (1, 9), (17, 19), (2, 2), (12, 50)]
    return [torch.from_numpy(make_frame(("photo", "noise", "ramp", "blocks")[i % 4], h, w, i)).to(DEV) for i, (h, w) in enumerate(sizes)]


def test_mixed_suffixes_return_what_the_four_modules_return_alone(frames):
    got = F.encode(frames, SUFFIXES)
    assert len(got) == len(frames) and all(isinstance(f, bytes) for f in got)
    for fmt, fn in ALONE.items():
        idx = [i for i, s in enumerate(SUFFIXES) if F.SUFFIX_FORMAT[s.lower()] == fmt]
        assert len(idx) >= 2
        assert [got[i] for i in idx] == fn([frames[i] for i in idx]).files(), fmt
    assert got[0][:2] == b"\xff\xd8" and got[1][:4] == b"II*\0" and got[2][:8] == M.png.SIGNATURE and got[3][:2] == b"BM"


def test_per_format_arguments_and_rectangles(frames):
    rects = np.array([[2, 3, 5, 30, 28], [0, 0, 0, 24, 16], [5, 7, 0, 8, 40], [2, 0, 11, 47, 12]])
    suffixes = [".tif", ".jpg", ".bmp", ".png"]
    got = F.encode(frames, suffixes, rects=rects, tiff=dict(rows_per_strip=1, predictor=False), jpeg=dict(quality=80), png=dict(filter="up"))
    assert got[0] == tiff_encode.encode(frames, rects=rects[:1], rows_per_strip=1, predictor=False).files()[0]
    assert got[1] == jpeg_encode.encode(frames, quality=80, rects=rects[1:2]).files()[0]
    assert got[2] == bmp_encode.encode(frames, rects=rects[2:3]).files()[0]
    assert got[3] == png_encode.encode(frames, "up", rects=rects[3:]).files()[0]
    assert F.encode(torch.stack([frames[4], frames[4]]), [".bmp", ".tif"]) == [bmp_encode.encode([frames[4]]).files()[0], tiff_encode.encode([frames[4]]).files()[0]]


def test_a_suffix_without_a_device_encoder_raises_by_name(frames, monkeypatch):
    def no_encoder(*a, **k):
        raise AssertionError("an encoder was reached")
    monkeypatch.setattr(F, "ENCODERS", {k: no_encoder for k in F.ENCODERS})
    for bad in (".webp", ".dng", ".WEBP", "", "tif", None):
        with pytest.raises(M.MafError, match="no device encoder") as e:
            F.encode(frames[:2], [".jpg", bad])
        assert repr(bad) in str(e.value) and "file 1" in str(e.value)
    with pytest.raises(M.MafError, match="2 suffixes for 3 files"):
        F.encode(frames[:3], [".jpg", ".png"])
    with pytest.raises(M.MafError, match="per-format"):
        F.encode(frames[:1], [".jpg"], webp=dict())
