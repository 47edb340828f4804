"""-m gpu: PNG encoding on the device (csrc/png_encode.hip, maf-yolo_amd/png_encode.py) against the files the interpreter's zlib module wrote
into tests/golden/png_encode_cases.npz and against the rule book (tests/png_encode_ref.py).  Byte-exact: ==, no tolerance.

* every fixture case (1x1, 1xN, Nx1 ... 64x64; noise, flat, ramp, photo, blocks) in one call per filter, and each alone;
* the targeted streams of png_encode_ref.targeted_frames (symbol counts around 16383 with the empty last block, run remainders, runs across rows
  and blocks, forced distance codes, fixed, stored, stored behind dynamic, gen_bitlen's repair at 15 and at 7 bits), each alone and all in one
  call; these frames are larger than 64 x 64 where their property needs 16383 symbols (up to 40 x 276, or one row of up to 2254 pixels);
* the taps (filtered bytes, tokens, block types, symbol counts, bit lengths, bit offsets, the packed stream) equal the rule book's, so a byte
  mismatch points at its stage;
* the 480 x 640 frame by the SHA-256 of its file;
* batch A, batch B, batch A again (stale bits in buffers the allocator hands back), a second stream, a pitched view, a [B, h, w, 3] tensor;
* rectangles (odd origins, touching the edges, one pixel wide or high) equal the encode of the sliced contiguous crops, for every filter;
* round trip: png.decode of the files on the device and png_ref.decode on the host return the frames;
* bad arguments raise MafError before the library is called;
* a noise frame whose stream comes within a few bytes of the output bound completes with a correct file.
"""
import hashlib

import numpy as np
import pytest
import torch

import png_encode_ref as R
import png_ref
import maf_yolo_amd as M
from maf_yolo_amd import png_encode as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILTER_NAMES = {v: k for k, v in R.FILTERS.items()}


@pytest.fixture(scope="module")
def cases(golden):
    """(name, frame on the device, host frame, the fixture's file) per case, grouped by filter: one call takes one filter."""
    z = golden("png_encode_cases")
    groups = {}
    for name, (h, w, ft) in zip((str(n) for n in z["names"]), z["meta"].tolist()):
        host = z["frame_%dx%d_%s" % (h, w, name.split("_")[1])]
        groups.setdefault(FILTER_NAMES[ft], []).append((name, torch.from_numpy(host).to(DEV), host, z["file_" + name].tobytes()))
    return groups, z


@pytest.fixture(scope="module")
def batches(cases):
    """Every filter's cases encoded in ONE call, with the taps (shared by the tests below; never modified)."""
    out = {}
    for filt, group in cases[0].items():
        taps = {}
        out[filt] = (E.encode([g[1] for g in group], filt, taps=taps), taps)
    return out


@pytest.fixture(scope="module")
def targeted():
    """(name, frame on the device, host frame, the rule book's file and taps) of every targeted stream; the reference is computed once."""
    out = []
    for name, host in R.targeted_frames().items():
        ref = {}
        want = R.encode(host, "sub", ref)
        out.append((name, torch.from_numpy(host).to(DEV), host, want, ref))
    return out


def check_taps(name, taps, k, ref):
    """The intermediate buffers of file `k` of a call against the rule book's taps `ref`."""
    job = taps["jobs"][k]
    n, r0 = int(job["n_raw"]), int(job["raw_off"])
    assert n == len(ref["raw"]), name
    assert np.array_equal(taps["raw"][r0:r0 + n].cpu().numpy(), ref["raw"]), "%s: filtered bytes" % name
    n_sym = int(taps["sums"][4 * k + 3])
    assert n_sym == len(ref["tokens"]), "%s: symbol count" % name
    assert np.array_equal(taps["tok"][r0:r0 + n_sym].cpu().numpy().view(np.uint16), ref["tokens"]), "%s: tokens" % name
    table = taps["blocks"].cpu().numpy().view(E.BLOCK_DT)[int(job["block0"]):int(job["block0"]) + int(job["n_blocks"])]
    used = table[:len(ref["blocks"])]
    assert (table[len(ref["blocks"]):]["type"] == E.UNUSED).all(), "%s: blocks behind the last" % name
    assert used["type"].tolist() == [b[0] for b in ref["blocks"]], "%s: block types" % name
    assert used["n_sym"].tolist() == [b[2] for b in ref["blocks"]], "%s: symbols per block" % name
    assert used["bits"].tolist() == [b[3] for b in ref["blocks"]], "%s: bit lengths" % name
    assert used["bitoff"].tolist() == ref["bitoff"], "%s: bit offsets" % name
    z = ref["zstream"]
    p0 = int(job["packed_off"])
    region = taps["packed"][p0:p0 + int(job["packed_bytes"])].cpu().numpy()
    assert bytes(region[2:len(z) - 4]) == z[2:-4], "%s: the packed stream" % name        # 78 01 and the Adler-32 are written by the copy
    assert not region[len(z) - 4:].any() and not region[:2].any(), "%s: bits outside the stream" % name


def test_every_case_in_one_call_per_filter_is_byte_exact(cases, batches):
    assert set(cases[0]) == set(R.FILTERS)
    for filt, group in cases[0].items():
        enc = batches[filt][0]
        assert enc.buffer.is_cuda and enc.lengths.dtype == torch.int32 and len(enc) == len(group)
        files = enc.files()
        assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
        for (name, _, _, want), got in zip(group, files):
            assert got == want, name
        assert enc.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone_is_byte_exact(cases):
    for filt, group in cases[0].items():
        for name, frame, _, want in group:
            assert E.encode([frame], filt).files() == [want], name


def test_each_targeted_stream_alone_is_byte_exact(targeted):
    for name, frame, _, want, _ in targeted:
        assert E.encode([frame]).files() == [want], name


def test_targeted_streams_in_one_call_and_their_taps(targeted):
    taps = {}
    files = E.encode([t[1] for t in targeted], "sub", taps=taps).files()
    for k, (name, _, _, want, ref) in enumerate(targeted):
        check_taps(name, taps, k, ref)
        assert files[k] == want, name


def test_taps_equal_the_rule_book(cases, batches):
    for filt, group in cases[0].items():
        taps = batches[filt][1]
        for k, (name, _, host, _) in enumerate(group):
            ref = {}
            R.encode(host, filt, ref)
            check_taps(name, taps, k, ref)


def test_large_frame_by_sha256(cases):
    frame = torch.from_numpy(R.large_frame()).to(DEV)
    got = E.encode([frame]).files()[0]
    assert hashlib.sha256(got).hexdigest() == str(cases[1]["large_sha256"])


def test_batch_a_then_b_then_a_again(cases):
    a, b = cases[0]["sub"], cases[0]["paeth"]
    first = E.encode([g[1] for g in a], "sub").files()
    other = E.encode([g[1] for g in b], "paeth").files()
    third = E.encode([g[1] for g in a], "sub").files()
    assert first == third == [g[3] for g in a]
    assert other == [g[3] for g in b]


def test_second_stream_gives_the_same_files(cases):
    group = cases[0]["sub"]
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)                            # the frames were uploaded on the default stream
    enc = E.encode([g[1] for g in group], stream=s)
    assert enc.files() == [g[3] for g in group]


def test_pitched_view_and_batched_tensor(cases):
    group = cases[0]["up"]
    for name, frame, _, want in group[-6:]:
        h, w = frame.shape[:2]
        wide = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device=DEV)
        wide[:, :w] = frame
        view = wide[:, :w]
        assert view.stride(0) == 3 * (w + 5) and (h == 1 or not view.is_contiguous())
        assert E.encode([view], "up").files() == [want], name
    same = [g for g in cases[0]["sub"] if g[0].startswith("8x8_")]
    stack = torch.stack([g[1] for g in same])              # [5, 8, 8, 3]
    assert E.encode(stack).files() == [g[3] for g in same]


def test_rectangles_equal_the_sliced_crops():
    rng = np.random.default_rng(7)
    f0 = torch.from_numpy(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)).to(DEV)
    f1 = torch.from_numpy(R.make_frame("blocks", 24, 40, 5)).to(DEV)
    rects = np.array([
        [0, 3, 5, 30, 28],       # odd x and y
        [0, 0, 0, 53, 37],       # the whole frame: touches every edge
        [0, 36, 1, 53, 37],      # right and bottom edge
        [1, 7, 0, 8, 24],        # 1 pixel wide
        [1, 0, 11, 40, 12],      # 1 pixel high
        [1, 39, 23, 40, 24],     # the last pixel
        [1, 5, 3, 21, 19],       # 16 x 16 at an odd origin
    ])
    frames = [f0, f1]
    crops = [frames[i][y1:y2, x1:x2].contiguous() for i, x1, y1, x2, y2 in rects.tolist()]
    for filt in R.FILTERS:
        got = E.encode(frames, filt, rects=rects).files()
        assert got == E.encode(crops, filt).files()
        for c, f in zip(crops, got):                       # and the crops themselves equal the rule book
            assert f == R.encode(c.cpu().numpy(), filt)


def test_round_trip_through_the_device_decoder_and_the_host_one(cases, batches, targeted):
    for filt, group in cases[0].items():
        files = batches[filt][0].files()
        frames = M.png.decode(files, device=DEV)
        for (name, frame, host, _), got, data in zip(group, frames, files):
            assert torch.equal(got, frame), name
            assert np.array_equal(png_ref.decode(data), host), name
    files = E.encode([t[1] for t in targeted]).files()
    for (name, frame, _, _, _), got in zip(targeted, M.png.decode(files, device=DEV)):
        assert torch.equal(got, frame), name


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
    with pytest.raises(M.MafError, match="rects"):
        E.encode([good], rects=np.array([[0.0, 0, 0, 4, 4]]))
    for filt in ("adaptive", "Sub", 1, None):
        with pytest.raises(M.MafError, match="filter"):
            E.encode([good], filter=filt)
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(1, 65536, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(65536, 1, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="uint8"):
        E.encode([good.float()])
    with pytest.raises(M.MafError, match="stride"):
        E.encode([torch.zeros(8, 3, 8, dtype=torch.uint8, device=DEV).permute(0, 2, 1)])
    with pytest.raises(M.MafError, match="no frames"):
        E.encode([])


def test_noise_at_the_output_bound_completes():
    """3 * 16383 - 1 filtered bytes of noise: three stored blocks, each 5 bytes beside its data where the bound allows 6, so the stream ends within
    10 bytes of the buffer's end; a second file behind it shows that nothing was written past the first one's share."""
    w = 2730                                               # 1 + 3 * w = 8191, 6 rows: 49146 = 3 * 16383 - 3 bytes
    rng = np.random.default_rng(12)
    noise = rng.integers(0, 256, (6, w, 3), dtype=np.uint8)
    other = R.make_frame("ramp", 5, 7, 1)
    enc = E.encode([torch.from_numpy(noise).to(DEV), torch.from_numpy(other).to(DEV)])
    files = enc.files()
    assert files == [R.encode(noise), R.encode(other)]
    slack = E._worst_case_bytes(6 * 8191) + E.FILE_BYTES - len(files[0])
    assert 0 <= slack <= 12
    assert np.array_equal(png_ref.decode(files[0]), noise)
