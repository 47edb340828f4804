"""-m gpu: lossless WebP encoding on the device (csrc/webp_encode.hip, maf-yolo_amd/webp_encode.py) against the files the rule book
(tests/webp_encode_ref.py) wrote into tests/golden/webp_encode_cases.npz.  Byte-exact: ==, no tolerance.

* every fixture case (1x1, 1xN, Nx1 ... 64x64; noise, flat, ramp, photo, blocks, smooth; predictor_bits 2, 3, 4) in one call per
  predictor_bits, and each alone;
* the targeted streams of webp_encode_ref.targeted_frames (tiny and one pixel wide or high frames up to a side of 16384, block edges plus one,
  run remainders around 4096, runs across rows and chunks, codes of one and two symbols, the 15-bit and the 7-bit repair, TR-reading modes in
  the last block column, the clamping modes, red and blue below green, predictor_bits 2 and 9), each alone and all in one call per bits;
* the taps (ARGB, modes, residuals, tokens, histograms, code lengths and codes, bit counts and offsets, the packed stream) equal the rule
  book's, so a byte mismatch points at its stage;
* the 480 x 640 frame by the SHA-256 of its file;
* batch A, batch B, batch A again (stale bits in buffers the allocator hands back), a second stream, a pitched view, a [B, h, w, 3] tensor;
* rectangles (odd origins, touching the edges, one pixel wide or high) equal the encode of the sliced contiguous crops;
* round trip: webp.decode of the files on the device and Pillow on the host return the frames;
* a noise frame, whose stream comes closest to the derived bound, completes with a correct file inside the bound;
* frames.encode with webp_lossless=True returns, per file, what each encoder returns alone; without it .webp is still refused.
"""
import hashlib
import io

import numpy as np
import pytest
import torch

import webp_encode_ref as R
from maf_yolo_amd import frames as F, jpeg_encode, png_encode, webp, webp_encode as E
from maf_yolo_amd.lib import MafError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _group(z, names_key, bits_key, prefix):
    """{bits: [(name, frame on the device, host frame, the fixture's file)]}: one call takes one predictor_bits."""
    groups = {}
    for name, bits in zip((str(n) for n in z[names_key]), z[bits_key].tolist()):
        host = z[prefix + "frame_" + name]
        groups.setdefault(bits, []).append((name, torch.from_numpy(host).to(DEV), host, z[prefix + "file_" + name].tobytes()))
    return groups


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("webp_encode_cases")
    return _group(z, "names", "bits", ""), z


@pytest.fixture(scope="module")
def targeted(cases):
    """The targeted frames as the fixture holds them (the host test pins them to webp_encode_ref.targeted_frames())."""
    return _group(cases[1], "targeted", "t_bits", "t_")


@pytest.fixture(scope="module")
def batches(cases):
    """Every predictor_bits' cases encoded in ONE call, with the taps (shared by the tests below; never modified)."""
    out = {}
    for bits, group in cases[0].items():
        taps = {}
        out[bits] = (E.encode([g[1] for g in group], bits, taps=taps), taps)
    return out


def check_taps(name, taps, k, host, bits):
    """The intermediate buffers of file `k` of a call against the rule book's taps, stage by stage."""
    ref = {}
    R.encode(host, bits, ref)
    job, images = taps["jobs"][k], taps["images"]
    n_files = len(taps["jobs"])
    main = images[2 * k + 1]
    o, n = int(main["px_off"]), int(main["n_px"])
    assert np.array_equal(taps["argb"][o:o + n].cpu().numpy().view(np.uint32), ref["argb"]), "%s: ARGB" % name
    b0, nb = int(job["block0"]), int(job["n_blocks"])
    assert np.array_equal(taps["modes"][b0:b0 + nb].cpu().numpy(), ref["modes"]), "%s: modes" % name
    sums = taps["sums"].cpu().numpy().reshape(2 * n_files, 4)
    hist = taps["hist"].cpu().numpy().reshape(2 * n_files, E.CODES, E.CODE_WORDS)
    codes = taps["codes"].cpu().numpy().view(np.uint32).reshape(2 * n_files, E.CODES, E.CODE_WORDS)
    cinfo = taps["cinfo"].cpu().numpy().reshape(2 * n_files, 8)
    for s, what in enumerate(("sub-image", "main image")):
        i, im, r = 2 * k + s, images[2 * k + s], ref["images"][s]
        o, n = int(im["px_off"]), int(im["n_px"])
        assert np.array_equal(taps["px"][o:o + n].cpu().numpy().view(np.uint32), r["px"]), "%s: pixels of the %s" % (name, what)
        assert sums[i, 0] == len(r["tokens"]), "%s: token count of the %s" % (name, what)
        assert np.array_equal(taps["tok"][o:o + len(r["tokens"])].cpu().numpy().view(np.uint32), r["tokens"]), "%s: tokens of the %s" % (name, what)
        for c, a in enumerate(R.ALPHABETS):
            assert np.array_equal(hist[i, c, :a], r["hist"][c]), "%s: histogram %d of the %s" % (name, c, what)
            assert np.array_equal(codes[i, c, :a] >> 16, r["lengths"][c]), "%s: code lengths %d of the %s" % (name, c, what)
            assert np.array_equal(codes[i, c, :a] & 0xffff, r["codes"][c]), "%s: codes %d of the %s" % (name, c, what)
        assert cinfo[i, :5].tolist() == r["head_bits"], "%s: description bits of the %s" % (name, what)
        assert sums[i, 1:].tolist() == [sum(r["head_bits"]), r["data_bits"], r["bitoff"]], "%s: bit counts and offset of the %s" % (name, what)
    p0 = int(job["packed_off"])
    region = taps["packed"][p0:p0 + int(job["packed_bytes"])].cpu().numpy()
    z = ref["payload"]
    assert bytes(region[:len(z)]) == z, "%s: the packed stream" % name
    assert not region[len(z):].any(), "%s: bits outside the stream" % name


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def test_every_case_in_one_call_per_bits_is_byte_exact(cases, batches):
    assert set(cases[0]) == {2, 3, 4} and len(cases[0][4]) >= 48
    for bits, group in cases[0].items():
        enc, taps = batches[bits]
        assert enc.buffer.is_cuda and enc.lengths.dtype == torch.int32 and len(enc) == len(group)
        files = enc.files()
        assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
        for k, ((name, _, host, want), got) in enumerate(zip(group, files)):
            check_taps(name, taps, k, host, bits)
            assert got == want, name
        assert enc.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone_is_byte_exact(cases):
    for bits, group in cases[0].items():
        for name, frame, _, want in group:
            assert E.encode([frame], bits).files() == [want], name


def test_each_targeted_stream_alone_is_byte_exact(targeted):
    assert sum(len(g) for g in targeted.values()) >= 26 and set(targeted) == {2, 4, 9}
    for bits, group in targeted.items():
        for name, frame, _, want in group:
            assert E.encode([frame], bits).files() == [want], name


def test_targeted_streams_in_one_call_and_their_taps(targeted):
    for bits, group in targeted.items():
        taps = {}
        files = E.encode([g[1] for g in group], bits, taps=taps).files()
        for k, (name, _, host, want) in enumerate(group):
            check_taps(name, taps, k, host, bits)
            assert files[k] == want, name


def test_large_frame_by_sha256(cases):
    frame = torch.from_numpy(R.large_frame()).to(DEV)
    got = E.encode([frame]).files()[0]
    assert len(got) == int(cases[1]["large_bytes"])
    assert hashlib.sha256(got).hexdigest() == str(cases[1]["large_sha256"])


def test_batch_a_then_b_then_a_again(cases):
    a, b = cases[0][4], cases[0][2]
    first = E.encode([g[1] for g in a], 4).files()
    other = E.encode([g[1] for g in b], 2).files()
    third = E.encode([g[1] for g in a], 4).files()
    assert first == third == [g[3] for g in a]
    assert other == [g[3] for g in b]


def test_a_second_stream_a_pitched_view_and_a_batch_tensor(cases):
    group = cases[0][4]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    assert E.encode([g[1] for g in group], stream=side).files() == [g[3] for g in group]
    name, _, host, want = next(g for g in group if g[0] == "33x47_photo_bits4")
    wide = torch.zeros(33, 64, 3, dtype=torch.uint8, device=DEV)
    wide[:, 9:56] = torch.from_numpy(host).to(DEV)
    view = wide[:, 9:56]
    assert not view.is_contiguous() and E.encode([view]).files() == [want]
    same = [g for g in group if g[2].shape == (17, 19, 3)]
    assert len(same) >= 5 and E.encode(torch.stack([g[1] for g in same])).files() == [g[3] for g in same]


def test_rectangles_equal_the_encode_of_the_crops(cases):
    group = cases[0][4]
    big = [next(g for g in group if g[0] == n) for n in ("64x64_photo_bits4", "33x47_blocks_bits4")]
    rects = np.array([[0, 0, 0, 64, 64], [0, 1, 3, 30, 40], [0, 63, 0, 64, 64], [0, 0, 63, 64, 64], [0, 17, 5, 18, 6], [1, 5, 7, 47, 33], [1, 0, 0, 1, 33],
                      [1, 46, 32, 47, 33], [1, 11, 1, 28, 18]])
    for bits in (4, 2):
        got = E.encode([g[1] for g in big], bits, rects=rects).files()
        for (f, x1, y1, x2, y2), data in zip(rects.tolist(), got):
            crop = np.ascontiguousarray(big[f][2][y1:y2, x1:x2])
            assert data == R.encode(crop, bits), (bits, f, x1, y1, x2, y2)


def test_round_trips_on_the_device_and_through_pillow(cases, batches, targeted):
    for bits, group in cases[0].items():
        files = batches[bits][0].files()
        back = webp.decode(files, device=DEV)
        for (name, frame, host, _), data, got in zip(group, files, back):
            assert torch.equal(got, frame), name
            assert np.array_equal(pillow_decode(data), host), name
    group = [g for g in targeted[4] if max(g[2].shape) <= 64]
    files = E.encode([g[1] for g in group]).files()
    for (name, frame, _, _), got in zip(group, webp.decode(files, device=DEV)):
        assert torch.equal(got, frame), name


def test_a_noise_frame_completes_inside_the_bound():
    host = np.random.default_rng(17).integers(0, 256, (97, 131, 3), dtype=np.uint8)
    for bits in (2, 4):
        taps = {}
        data = E.encode([torch.from_numpy(host).to(DEV)], bits, taps=taps).files()[0]
        assert data == R.encode(host, bits)
        assert np.array_equal(pillow_decode(data), host)
        nb = int(taps["jobs"][0]["n_blocks"])
        bound = E._worst_case_bytes(97 * 131, nb)
        assert 3 * 97 * 131 <= len(data) - E.FILE_BYTES <= bound <= int(taps["jobs"][0]["packed_bytes"])      # noise: 24 of the 45 provable bits per pixel


def test_bad_arguments_raise_before_the_library_is_called():
    f = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    for bits in (1, 10, 4.0, True, None):
        with pytest.raises(MafError, match="predictor_bits"):
            E.encode([f], bits)
    with pytest.raises(MafError, match="16384"):
        E.encode([torch.zeros(1, 16385, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(MafError, match="empty"):
        E.encode([torch.zeros(0, 4, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(MafError, match="no frames"):
        E.encode([])
    assert len(E.encode([torch.zeros(1, 16385, 3, dtype=torch.uint8, device=DEV)], rects=np.array([[0, 1, 0, 16385, 1]])).files()[0]) > 20


def test_the_router_sends_webp_files_to_this_encoder(cases):
    group = cases[0][4]
    four = [next(g for g in group if g[0] == n) for n in ("17x19_photo_bits4", "33x47_ramp_bits4", "8x8_noise_bits4", "64x64_smooth_bits4")]
    fr = [g[1] for g in four]
    suffixes = [".jpg", ".webp", ".png", ".WEBP"]
    got = F.encode(fr, suffixes, webp_lossless=True)
    assert got == [jpeg_encode.encode([fr[0]]).files()[0], four[1][3], png_encode.encode([fr[2]]).files()[0], four[3][3]]
    assert F.encode(fr, suffixes, webp_lossless=dict(predictor_bits=3))[1] == R.encode(four[1][2], 3)
    with pytest.raises(MafError, match="no device encoder"):
        F.encode(fr, suffixes)
    with pytest.raises(MafError, match="per-format arguments are"):
        F.encode(fr, suffixes, webp={})
