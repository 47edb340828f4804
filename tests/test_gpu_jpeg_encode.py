"""-m gpu: baseline JPEG encoding on the device (csrc/jpeg_encode.hip, maf-yolo_amd/jpeg_encode.py) against the files Pillow
(libjpeg-turbo) wrote into tests/golden/jpeg_encode_cases.npz.  Byte-exact: ==, no tolerance.

* every case (1x1 ... 33x47; 4:2:0 and 4:4:4; quality 30 / 75 / 95 / 100; random, ramp and saturated content) alone and all in one call;
* the taps (coefficients in coded order, bits per block, the stream before stuffing) equal tests/jpeg_encode_ref.py, so a byte mismatch
  points at its stage;
* the 480 x 640 frame by the sha256 of its file;
* batch A, batch B, batch A again (stale bits in buffers the allocator hands back), a second stream, a pitched view, a [B, h, w, 3] tensor;
* rectangles (odd origins, touching the edges, one pixel wide or high) equal the encode of the sliced contiguous crops;
* jpeg.decode of the files equals Pillow's decode of the fixture files;
* bad arguments raise MafError before the library is called.
"""
import hashlib

import numpy as np
import pytest
import torch

import jpeg_encode_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import jpeg_encode as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SS = {2: "4:2:0", 1: "4:4:4"}


@pytest.fixture(scope="module")
def cases(golden):
    """(name, frame on the device, quality, subsampling, the fixture's file) per case, grouped by setting: one call takes one setting."""
    z = golden("jpeg_encode_cases")
    groups = {}
    for name, (h, w, hs, q) in zip((str(n) for n in z["names"]), z["meta"].tolist()):
        kind = name.split("_")[1]
        host = z["frame_%dx%d_%s" % (h, w, kind)]
        groups.setdefault((int(q), SS[hs]), []).append((name, torch.from_numpy(host).to(DEV), host, z["file_" + name].tobytes()))
    return groups, z


@pytest.fixture(scope="module")
def batches(cases):
    """Every setting's cases encoded in ONE call, with the taps (shared by the tests below; never modified)."""
    out = {}
    for key, group in cases[0].items():
        taps = {}
        out[key] = (E.encode([g[1] for g in group], key[0], key[1], taps=taps), taps)
    return out


def test_every_case_in_one_call_per_setting_is_byte_exact(cases, batches):
    for key, group in cases[0].items():
        enc = batches[key][0]
        assert enc.buffer.is_cuda and enc.lengths.dtype == torch.int32 and len(enc) == len(group)
        files = enc.files()
        assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
        for (name, _, _, want), got in zip(group, files):
            assert got == want, name
        assert enc.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone_is_byte_exact(cases):
    for (q, ss), group in cases[0].items():
        for name, frame, _, want in group:
            assert E.encode([frame], q, ss).files() == [want], name


def test_taps_equal_the_reference(cases, batches):
    for (q, ss), group in cases[0].items():
        enc, taps = batches[(q, ss)]
        coef = taps["coef"].cpu().numpy().reshape(-1, 64)
        bits = taps["bits"].cpu().numpy()
        bitoff = taps["bitoff"].cpu().numpy()
        packed = taps["packed"].cpu().numpy()
        assert bitoff[0] == 0 and np.array_equal(np.diff(bitoff), bits)
        for (name, _, host, _), job in zip(group, taps["jobs"]):
            ref = {}
            R.encode(host, q, ss, taps=ref)
            b0, nb, c0 = int(job["block0"]), int(job["n_blocks"]), int(job["chunk0"])
            assert nb == len(ref["coded"]), name
            assert np.array_equal(coef[b0:b0 + nb], ref["coded"]), "%s: coefficients" % name
            assert np.array_equal(bits[b0:b0 + nb], ref["bits"]), "%s: bits per block" % name
            n = len(ref["stream"])
            region = packed[c0 * E.CHUNK:(c0 + int(job["n_chunks"])) * E.CHUNK]
            assert np.array_equal(region[:n], ref["stream"]), "%s: the stream before stuffing" % name
            assert not region[n:].any(), "%s: bits behind the end of the stream" % name


def test_large_frame_by_sha256(cases):
    z = cases[1]
    frame = torch.from_numpy(R.smooth_frame(480, 640)).to(DEV)
    got = E.encode([frame], 95, "4:2:0").files()[0]
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(z["large_file"].tobytes()).hexdigest()


def test_batch_a_then_b_then_a_again(cases):
    a = cases[0][(100, "4:2:0")]
    b = cases[0][(30, "4:4:4")]
    first = E.encode([g[1] for g in a], 100, "4:2:0").files()
    other = E.encode([g[1] for g in b], 30, "4:4:4").files()
    third = E.encode([g[1] for g in a], 100, "4:2:0").files()
    assert first == third == [g[3] for g in a]
    assert other == [g[3] for g in b]


def test_second_stream_gives_the_same_files(cases):
    group = cases[0][(95, "4:2:0")]
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)                            # the frames were uploaded on the default stream
    enc = E.encode([g[1] for g in group], 95, "4:2:0", stream=s)
    assert enc.files() == [g[3] for g in group]


def test_pitched_view_and_batched_tensor(cases):
    group = cases[0][(75, "4:2:0")]
    for name, frame, _, want in group[-6:]:
        h, w = frame.shape[:2]
        wide = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device=DEV)
        wide[:, :w] = frame
        view = wide[:, :w]
        assert view.stride(0) == 3 * (w + 5) and (h == 1 or not view.is_contiguous())
        assert E.encode([view], 75, "4:2:0").files() == [want], name
    same = [g for g in group if g[0].startswith("16x16_")]
    stack = torch.stack([g[1] for g in same])              # [3, 16, 16, 3]
    assert E.encode(stack, 75, "4:2:0").files() == [g[3] for g in same]


def test_rectangles_equal_the_sliced_crops():
    rng = np.random.default_rng(7)
    f0 = torch.from_numpy(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)).to(DEV)
    f1 = torch.from_numpy(R.make_frame("saturated", 24, 40, 5)).to(DEV)
    rects = np.array([
        [0, 3, 5, 30, 28],       # odd x and y
        [0, 0, 0, 53, 37],       # the whole frame: touches every edge
        [0, 36, 1, 53, 37],      # right and bottom edge
        [1, 7, 0, 8, 24],        # 1 pixel wide
        [1, 0, 11, 40, 12],      # 1 pixel high
        [1, 39, 23, 40, 24],     # the last pixel
        [0, 1, 1, 18, 10],       # dummy block column and row in 4:2:0
        [1, 5, 3, 21, 19],       # 16 x 16 at an odd origin
    ])
    frames = [f0, f1]
    crops = [frames[i][y1:y2, x1:x2].contiguous() for i, x1, y1, x2, y2 in rects.tolist()]
    for q, ss in ((95, "4:2:0"), (100, "4:4:4")):
        got = E.encode(frames, q, ss, rects=rects).files()
        want = E.encode(crops, q, ss).files()
        assert got == want
        for c, f in zip(crops, got):                       # and the crops themselves equal the reference
            assert f == R.encode(c.cpu().numpy(), q, ss)


def test_round_trip_through_the_device_decoder(cases, batches):
    z = cases[1]
    for key, group in cases[0].items():
        frames = M.jpeg.decode(batches[key][0].files(), device=DEV)
        for (name, _, _, _), got in zip(group, frames):
            assert torch.equal(got.cpu(), torch.from_numpy(z["bgr_" + name])), name


def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(E, "_library", no_library)
    good = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(M.MafError, match="no CPU fallback"):
        E.encode([good.cpu()])
    with pytest.raises(M.MafError, match="no CPU fallback"):
        E.encode([good, good.cpu()])
    for empty in (torch.zeros(0, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(8, 0, 3, dtype=torch.uint8, device=DEV)):
        with pytest.raises(M.MafError, match="empty"):
            E.encode([empty])
    for rect in ([0, 2, 2, 2, 6], [0, 2, 6, 5, 6], [0, 5, 2, 3, 6]):
        with pytest.raises(M.MafError, match="empty"):
            E.encode([good], rects=np.array([rect]))
    for rect in ([0, -1, 0, 4, 4], [0, 0, 0, 9, 4], [0, 0, 0, 4, 9], [0, 0, -2, 4, 4]):
        with pytest.raises(M.MafError, match="outside"):
            E.encode([good], rects=np.array([rect]))
    with pytest.raises(M.MafError, match="names frame"):
        E.encode([good], rects=np.array([[1, 0, 0, 4, 4]]))
    for q in (0, 101, 95.5):
        with pytest.raises(M.MafError, match="quality"):
            E.encode([good], quality=q)
    with pytest.raises(M.MafError, match="subsampling"):
        E.encode([good], subsampling="4:2:2")
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(1, 65536, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(65536, 1, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="uint8"):
        E.encode([good.float()])
    with pytest.raises(M.MafError, match="stride"):
        E.encode([torch.zeros(8, 3, 8, dtype=torch.uint8, device=DEV).permute(0, 2, 1)])
