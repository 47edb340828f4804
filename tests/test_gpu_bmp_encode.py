"""-m gpu: BMP encoding on the device (csrc/bmp_encode.hip, maf-yolo_amd/bmp_encode.py) against Pillow's pixel arrays in
tests/golden/tiff_encode_cases.npz and the rule book (tests/bmp_encode_ref.py).  Byte-exact: ==, no tolerance.

* widths 1 to 9 and 64, heights 1 and 5 (every row padding; files that start at every alignment of the output), all in one call and each alone;
* the header field by field, the pixel array against Pillow's;
* a frame of more than one 4096-byte chunk, a pitched view, a [B, h, w, 3] tensor, a second stream, batch A / B / A;
* rectangles equal the encode of the sliced contiguous crops;
* bmp.decode on the device and bmp_ref.decode on the host return the frames; Pillow opens the files;
* bad arguments raise MafError before the library is called.
"""
import io

import numpy as np
import pytest
import torch

import bmp_encode_ref as R
import bmp_ref
from tiff_encode_ref import make_frame
import maf_yolo_amd as M
from maf_yolo_amd import bmp_encode as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    """(name, frame on the device, host frame, Pillow's pixel array) per BMP case of the fixture."""
    z = golden("tiff_encode_cases")
    out = []
    for name in (str(n) for n in z["bmp_names"]):
        size, seed = name.split("_")
        h, w = (int(v) for v in size.split("x"))
        host = make_frame("noise", h, w, int(seed))
        out.append((name, torch.from_numpy(host).to(DEV), host, z["bmp_" + name].tobytes()))
    return out


@pytest.fixture(scope="module")
def batch(cases):
    return E.encode([c[1] for c in cases])


def test_every_case_in_one_call(cases, batch):
    assert batch.buffer.is_cuda and batch.lengths.dtype == torch.int32 and len(batch) == len(cases)
    files = batch.files()
    for (name, _, host, want), got in zip(cases, files):
        h, w = host.shape[:2]
        assert got[54:] == want, name
        assert R.read_header(got) == dict(magic=b"BM", file_size=54 + R.row_stride(w) * h, reserved1=0, reserved2=0, pixel_offset=54, header_size=40,
                                          width=w, height=h, planes=1, bit_count=24, compression=0, image_size=0, x_pixels_per_metre=0,
                                          y_pixels_per_metre=0, colours_used=0, colours_important=0), name
        assert got == R.encode(host), name
    assert batch.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone(cases):
    for name, frame, host, _ in cases:
        assert E.encode([frame]).files() == [R.encode(host)], name


def test_frames_of_more_than_one_chunk_and_a_batched_tensor():
    hosts = [make_frame("photo", 41, 67, 1), make_frame("noise", 3, 1501, 2), make_frame("blocks", 70, 33, 3)]      # 8 KB, 13 KB, 7 KB
    files = E.encode([torch.from_numpy(f).to(DEV) for f in hosts]).files()
    assert files == [R.encode(f) for f in hosts]
    stack = torch.from_numpy(np.stack([make_frame("noise", 9, 7, s) for s in range(4)])).to(DEV)
    assert E.encode(stack).files() == [R.encode(f) for f in stack.cpu().numpy()]


def test_pitched_view_second_stream_and_a_b_a(cases, batch):
    for name, frame, host, _ in cases[8:14]:
        h, w = frame.shape[:2]
        wide = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device=DEV)
        wide[:, :w] = frame
        assert E.encode([wide[:, :w]]).files() == [R.encode(host)], name
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)                            # the frames were uploaded on the default stream
    assert E.encode([c[1] for c in cases], stream=s).files() == batch.files()
    a, b = cases[:10], cases[10:]
    first = E.encode([c[1] for c in a]).files()
    other = E.encode([c[1] for c in b]).files()
    assert E.encode([c[1] for c in a]).files() == first == [R.encode(c[2]) for c in a]
    assert other == [R.encode(c[2]) for c in b]


def test_rectangles_equal_the_sliced_crops():
    rng = np.random.default_rng(7)
    f0 = torch.from_numpy(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)).to(DEV)
    f1 = torch.from_numpy(make_frame("blocks", 24, 40, 5)).to(DEV)
    rects = np.array([[0, 3, 5, 30, 28], [0, 0, 0, 53, 37], [0, 36, 1, 53, 37], [1, 7, 0, 8, 24], [1, 0, 11, 40, 12], [1, 39, 23, 40, 24], [1, 5, 3, 21, 19]])
    frames = [f0, f1]
    crops = [frames[i][y1:y2, x1:x2].contiguous() for i, x1, y1, x2, y2 in rects.tolist()]
    got = E.encode(frames, rects=rects).files()
    assert got == E.encode(crops).files() == [R.encode(c.cpu().numpy()) for c in crops]


def test_round_trips(cases, batch):
    Image = pytest.importorskip("PIL.Image")
    files = batch.files()
    for (name, frame, host, _), got, data in zip(cases, M.bmp.decode(files, device=DEV), files):
        assert torch.equal(got, frame), name
        assert np.array_equal(bmp_ref.decode(data), host), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1], host), name


def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(E, "_library", no_library)
    good = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(M.MafError, match="no CPU fallback"):
        E.encode([good, good.cpu()])
    with pytest.raises(M.MafError, match="empty"):
        E.encode([torch.zeros(0, 8, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="empty"):
        E.encode([good], rects=np.array([[0, 2, 2, 2, 6]]))
    with pytest.raises(M.MafError, match="outside"):
        E.encode([good], rects=np.array([[0, 0, 0, 9, 4]]))
    with pytest.raises(M.MafError, match="65535 files"):
        E.encode([good], rects=np.tile(np.array([[0, 0, 0, 1, 1]]), (65536, 1)))
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(1, 65536, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="uint8"):
        E.encode([good.float()])
    with pytest.raises(M.MafError, match="no frames"):
        E.encode([])
