"""No GPU: the rule book of the BMP encoder (tests/bmp_encode_ref.py) against Pillow's pixel arrays in tests/golden/tiff_encode_cases.npz, the
readers, and the hand-written binding of maf-yolo_amd/bmp_encode.py.  Every comparison is ==.

* widths 1 to 9 and 64 (every row padding), heights 1 and 5: the pixel array equals Pillow's file[54:] from the fixture, and a fresh Pillow's
  where it imports;
* the header, field by field;
* bmp_ref.decode and Pillow read the files back to the exact pixels;
* the prototypes of include/mafyolo_bmp_encode.h equal the binding, outside lib.EXPORTS; the struct sizes equal the library's; a tampered blob
  is rejected on the host before any device pointer is used.
"""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import bmp_encode_ref as R
import bmp_ref
from tiff_encode_ref import make_frame
from maf_yolo_amd import bmp_encode as E, lib, staging
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    """(name, frame, Pillow's pixel array) per BMP case of the fixture."""
    z = golden("tiff_encode_cases")
    out = []
    for name in (str(n) for n in z["bmp_names"]):
        size, seed = name.split("_")
        h, w = (int(v) for v in size.split("x"))
        out.append((name, make_frame("noise", h, w, int(seed)), z["bmp_" + name].tobytes()))
    return out


def test_the_cases_cover_every_row_padding(cases):
    assert {c[1].shape[:2] for c in cases} == {(h, w) for h in (1, 5) for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64)}
    assert {R.row_stride(c[1].shape[1]) - 3 * c[1].shape[1] for c in cases} == {0, 1, 2, 3}


def test_pixel_array_equals_pillow(cases):
    for name, frame, want in cases:
        data = R.encode(frame)
        assert data[54:] == want, name
        assert len(data) == E.file_bytes(frame.shape[1], frame.shape[0]), name


def test_pixel_array_equals_a_fresh_pillow(cases):
    Image = pytest.importorskip("PIL.Image")
    for name, frame, want in cases:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, "BMP")
        assert buf.getvalue()[54:] == want == R.pixel_array(frame), name


def test_header_field_by_field(cases):
    for name, frame, _ in cases:
        h, w = frame.shape[:2]
        got = R.read_header(R.encode(frame))
        assert got == dict(magic=b"BM", file_size=54 + R.row_stride(w) * h, reserved1=0, reserved2=0, pixel_offset=54, header_size=40, width=w, height=h,
                           planes=1, bit_count=24, compression=0, image_size=0, x_pixels_per_metre=0, y_pixels_per_metre=0, colours_used=0,
                           colours_important=0), name


def test_readers_return_the_frames(cases):
    Image = pytest.importorskip("PIL.Image")
    for name, frame, _ in cases:
        data = R.encode(frame)
        assert np.array_equal(bmp_ref.decode(data), frame), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1], frame), name


def test_header_prototypes_equal_the_binding():
    text = open(os.path.join(ROOT, "include", "mafyolo_bmp_encode.h")).read()
    protos = dict(re.findall(r"^int (maf_bmp_\w+)\(([^;]*)\);", text, re.M | re.S))
    assert set(protos) == set(E.PROTOTYPES)
    for name, args in protos.items():
        res, argtypes = E.PROTOTYPES[name]
        assert res is ctypes.c_int32
        params = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            assert "*" in p or "stream_t" in p, (name, p)
            assert t is ctypes.c_void_p or t == ctypes.POINTER(ctypes.c_int32)
    hip = open(os.path.join(ROOT, "include", "mafyolo_hip.h")).read()
    for name in E.PROTOTYPES:
        assert name not in lib.EXPORTS and name not in hip
    assert int(re.search(r"#define MAF_BMP_ENC_CHUNK (\d+)", text).group(1)) == E.CHUNK
    assert int(re.search(r"#define MAF_BMP_ENC_HEAD_BYTES (\d+)", text).group(1)) == E.HEAD_BYTES == R.HEAD_BYTES


def test_struct_sizes_equal_the_library():
    L = E._library()
    sizes = (ctypes.c_int32 * 2)()
    assert L.maf_bmp_encode_struct_sizes(sizes) == 0
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize] == [32, 40]


def test_a_tampered_blob_is_rejected_on_the_host():
    L = E._library()
    w, h = 5, 4
    size = E.file_bytes(w, h)
    job = np.zeros(1, E.JOB_DT)
    job["src"], job["pitch"], job["w"], job["h"], job["n_chunks"] = 4096, 15, w, h, 1

    def call(jobs, **fields):
        hdr, off = staging.blob_layout(E.HEADER_DT, (("jobs_off", jobs),))
        hdr["n_files"], hdr["n_chunks"], hdr["total_bytes"], hdr["out_bytes"] = 1, 1, off, staging.align(size)
        for k, v in fields.items():
            hdr[k] = v
        buf = np.zeros(off, np.uint8)
        staging.write_blob(buf, hdr, (("jobs_off", jobs),))
        fake = 1 << 20                                                                  # never dereferenced: every call below fails validation first
        return L.maf_bmp_encode(buf.ctypes.data, *([fake] * 4), None)
    for field, value in (("w", 0), ("h", 70000), ("pitch", 14), ("out_off", 16), ("n_chunks", 2), ("chunk0", 1), ("src", 0)):
        bad = job.copy()
        bad[field] = value
        assert call(bad) != 0, field
        with pytest.raises(MafError):
            lib.check(call(bad))
    for field, value in (("n_files", 0), ("n_chunks", 2), ("out_bytes", size - 1), ("jobs_off", 8), ("total_bytes", 16)):
        assert call(job, **{field: value}) != 0, field
    with pytest.raises(MafError, match="smaller than the files"):                       # the job itself is in order: only the last check fails
        lib.check(call(job, out_bytes=size - 1))


def test_encode_refuses_cpu_frames_without_a_gpu():
    torch = pytest.importorskip("torch")
    with pytest.raises(MafError, match="no CPU fallback"):
        E.encode([torch.zeros(4, 4, 3, dtype=torch.uint8)])


def test_refusal_texts(monkeypatch):
    """The refusals encode() makes itself, by name and before the library is called."""
    torch = pytest.importorskip("torch")

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(E, "_library", no_library)
    monkeypatch.setattr(E.staging, "frame_list", lambda frames, text: list(frames))     # host tensors stand in: nothing below touches their memory
    good = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(MafError, match="takes up to 65535 files per call"):
        E.encode([good], rects=np.tile(np.array([[0, 0, 0, 1, 1]]), (65536, 1)))
    huge = torch.zeros(1, 1, 3, dtype=torch.uint8).expand(40000, 20000, 3)
    with pytest.raises(MafError, match="fewer than 2 GiB are taken"):
        E.encode([huge])
    monkeypatch.setattr(E.staging, "MAX_BLOB", 64)                                      # a header and one job are 80 bytes; 65535 jobs never reach 2 GiB
    with pytest.raises(MafError, match="the job table of one call is limited to 2 GiB"):
        E.encode([good])
