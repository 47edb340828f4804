"""-m gpu: TIFF encoding on the device (csrc/tiff_encode.hip, maf-yolo_amd/tiff_encode.py) against the strips Pillow / libtiff wrote into
tests/golden/tiff_encode_cases.npz and against the rule book (tests/tiff_encode_ref.py).  Byte-exact: ==, no tolerance.

* every fixture case (1x1, 1xN, Nx1 ... 64x64; noise, flat, ramp, photo, blocks) in one call and each alone, under the cv2 strip rule and with
  1, min(4, h) and h rows per strip: strips and tag values against the fixture, whole files against the rule book;
* the 480 x 640 frame by the SHA-256 of its strips, its file against the rule book's;
* the targeted frames of tiff_encode_ref.targeted_frames (EOI width bumps, a strip that ends as the table fills, one and two table-full resets,
  a ratio checkpoint that records and one that resets, a byte-aligned end and a padded one, 1 x 1), each alone and all in one call;
* the taps (differenced bytes, codes and widths, Clear positions, strip bit counts, lengths and offsets) equal the rule book's, so a byte
  mismatch points at its stage;
* predictor=False; batch A, batch B, batch A again (stale bytes in buffers the allocator hands back), a second stream, a pitched view, a
  [B, h, w, 3] tensor;
* rectangles (odd origins, touching the edges, one pixel wide or high) equal the encode of the sliced contiguous crops;
* round trip: tiff.decode of the files on the device returns the frames;
* bad arguments raise MafError before the library is called.
"""
import hashlib

import numpy as np
import pytest
import torch

import tiff_encode_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import tiff_encode as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TAGS = (256, 257, 259, 262, 277, 278, 284, 317)
MODES = ("cv2", "1", "4", "h", "nopred")


def tag_values(tags):
    return [tags.get(t, [0])[0] for t in TAGS] + tags[258]


@pytest.fixture(scope="module")
def cases(golden):
    """mode -> [(variant, frame on the device, host frame, rows per strip, the fixture's strips, its tag values)], one entry per frame and mode
    ("cv2": the strip rule, "1", "4": min(4, h), "h", "nopred": the strip rule without the predictor)."""
    z = golden("tiff_encode_cases")
    groups = {m: [] for m in MODES}
    for name, (h, w) in zip((str(n) for n in z["names"]), z["meta"].tolist()):
        host = z["frame_" + name]
        dev = torch.from_numpy(host).to(DEV)
        rows = {"cv2": R.cv2_rows_per_strip(w, h), "1": 1, "4": min(4, h), "h": h, "nopred": R.cv2_rows_per_strip(w, h)}
        for mode, r in rows.items():
            variant = name + ("_nopred" if mode == "nopred" else "_r%d" % r)
            lens = z["lens_" + variant].tolist()
            blob = z["strips_" + variant].tobytes()
            ends = np.cumsum(lens).tolist()
            groups[mode].append((variant, dev, host, r, [blob[e - n:e] for e, n in zip(ends, lens)], z["tags_" + variant].tolist()))
    return groups, z


def encode_group(group, mode, **kw):
    if mode == "cv2":
        return E.encode([g[1] for g in group], **kw)
    if mode == "nopred":
        return E.encode([g[1] for g in group], predictor=False, **kw)
    return E.encode([g[1] for g in group], rows_per_strip=[g[3] for g in group], **kw)


@pytest.fixture(scope="module")
def batches(cases):
    """Every mode's cases encoded in ONE call, with the taps (shared by the tests below; never modified)."""
    out = {}
    for mode, group in cases[0].items():
        taps = {}
        out[mode] = (encode_group(group, mode, taps=taps), taps)
    return out


@pytest.fixture(scope="module")
def targeted():
    """(name, frame on the device, host frame, the rule book's file and taps) of every targeted frame; the reference is computed once."""
    out = []
    for name, host in R.targeted_frames().items():
        ref = {}
        want = R.encode(host, taps=ref)
        out.append((name, torch.from_numpy(host).to(DEV), host, want, ref))
    return out


def check_taps(name, taps, k, ref, data):
    """The intermediate buffers of file `k` of a call against the rule book's taps `ref`; `data`: the file the device wrote."""
    job = taps["jobs"][k]
    n = 3 * int(job["w"]) * int(job["h"])
    r0 = int(job["raw_off"])
    assert n == len(ref["raw"]), name
    assert np.array_equal(taps["raw"][r0:r0 + n].cpu().numpy(), ref["raw"]), "%s: differenced bytes" % name
    assert int(job["n_strips"]) == len(ref["strips"]) and int(job["rows_per_strip"]) == ref["rows_per_strip"], "%s: strips" % name
    table = taps["strips"].cpu().numpy().view(E.STRIP_DT)[int(job["strip0"]):int(job["strip0"]) + int(job["n_strips"])]
    assert table["n_codes"].tolist() == [len(t["codes"]) for t in ref["strips"]], "%s: codes per strip" % name
    assert table["bits"].tolist() == [t["bits"] for t in ref["strips"]], "%s: bits per strip" % name
    codes = taps["codes"].cpu().numpy().view(np.uint16)
    for s, t in enumerate(ref["strips"]):
        c0 = int(job["code_off"]) + s * int(job["code_slot"])
        got = codes[c0:c0 + len(t["codes"])]
        assert (got & 0xFFF).tolist() == t["codes"], "%s: codes of strip %d" % (name, s)
        assert (9 + (got >> 12)).tolist() == t["widths"], "%s: code widths of strip %d" % (name, s)
        assert np.flatnonzero((got & 0xFFF) == R.CLEAR).tolist() == t["clears"], "%s: Clear positions of strip %d" % (name, s)
    assert table["bytes"].tolist() == ref["lengths"], "%s: strip lengths" % name
    assert table["offset"].tolist() == ref["offsets"], "%s: strip offsets" % name
    for s, (o, m) in enumerate(zip(ref["offsets"], ref["lengths"])):
        assert data[o:o + m] == R.lzw(ref["raw"][s * ref["rows_per_strip"] * 3 * int(job["w"]):][:3 * int(job["w"]) * ref["rows_per_strip"]].tobytes()), \
            "%s: packed bytes of strip %d" % (name, s)


def test_every_case_in_one_call_per_mode_is_byte_exact(cases, batches):
    for mode, group in cases[0].items():
        enc = batches[mode][0]
        assert enc.buffer.is_cuda and enc.lengths.dtype == torch.int32 and len(enc) == len(group)
        files = enc.files()
        assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
        for (variant, _, host, r, want, tags), got in zip(group, files):
            got_tags, strips = R.file_strips(got)
            assert strips == want, variant                                               # libtiff's strips
            assert tag_values(got_tags) == tags, variant                                 # and its tag values
            assert got == R.encode(host, r, mode != "nopred"), variant                   # the file around them: the rule book's
        assert enc.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone_is_byte_exact(cases):
    for mode, group in cases[0].items():
        for g in group:
            got, = encode_group([g], mode).files()
            assert R.file_strips(got)[1] == g[4], g[0]
            assert got == R.encode(g[2], g[3], mode != "nopred"), g[0]


def test_integer_rows_per_strip_applies_to_every_file(cases):
    group = [g for g in cases[0]["4"] if g[3] == 4]
    assert len(group) >= 20
    files = E.encode([g[1] for g in group], rows_per_strip=4).files()
    assert [R.file_strips(f)[1] for f in files] == [g[4] for g in group]


def test_large_frame_by_sha256(cases):
    host = R.large_frame()
    taps = {}
    got = E.encode([torch.from_numpy(host).to(DEV)], taps=taps).files()[0]
    tags, strips = R.file_strips(got)
    assert [len(s) for s in strips] == cases[1]["large_lens"].tolist()
    assert hashlib.sha256(b"".join(strips)).hexdigest() == str(cases[1]["large_sha256"])
    assert tag_values(tags) == cases[1]["large_tags"].tolist()
    ref = {}
    assert got == R.encode(host, taps=ref)
    check_taps("large", taps, 0, ref, got)


def test_each_targeted_frame_alone_is_byte_exact(targeted):
    for name, frame, _, want, _ in targeted:
        assert E.encode([frame]).files() == [want], name


def test_targeted_frames_in_one_call_and_their_taps(targeted):
    taps = {}
    files = E.encode([t[1] for t in targeted], taps=taps).files()
    for k, (name, _, _, want, ref) in enumerate(targeted):
        check_taps(name, taps, k, ref, files[k])
        assert files[k] == want, name


def test_taps_equal_the_rule_book(cases, batches):
    for mode in ("cv2", "1", "nopred"):
        enc, taps = batches[mode]
        files = enc.files()
        for k, (variant, _, host, r, _, _) in enumerate(cases[0][mode]):
            ref = {}
            R.encode(host, r, mode != "nopred", ref)
            check_taps(variant, taps, k, ref, files[k])


def test_batch_a_then_b_then_a_again(cases):
    a, b = cases[0]["cv2"], cases[0]["1"]
    first = encode_group(a, "cv2").files()
    other = encode_group(b, "1").files()
    third = encode_group(a, "cv2").files()
    assert first == third == [R.encode(g[2], g[3]) for g in a]
    assert other == [R.encode(g[2], g[3]) for g in b]


def test_second_stream_gives_the_same_files(cases, batches):
    group = cases[0]["cv2"]
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)                            # the frames were uploaded on the default stream
    enc = E.encode([g[1] for g in group], stream=s)
    assert enc.files() == batches["cv2"][0].files()


def test_pitched_view_and_batched_tensor(cases):
    group = cases[0]["cv2"]
    for variant, frame, host, r, _, _ in group[-6:]:
        h, w = frame.shape[:2]
        wide = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device=DEV)
        wide[:, :w] = frame
        view = wide[:, :w]
        assert view.stride(0) == 3 * (w + 5) and (h == 1 or not view.is_contiguous())
        assert E.encode([view]).files() == [R.encode(host, r)], variant
    same = [g for g in group if g[0].startswith("8x8_")]
    stack = torch.stack([g[1] for g in same])              # [5, 8, 8, 3]
    assert E.encode(stack).files() == [R.encode(g[2], g[3]) for g in same]


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
    for kw in ({}, {"rows_per_strip": 1}, {"predictor": False}):
        got = E.encode(frames, rects=rects, **kw).files()
        assert got == E.encode(crops, **kw).files()
        for c, f in zip(crops, got):                       # and the crops themselves equal the rule book
            assert f == R.encode(c.cpu().numpy(), kw.get("rows_per_strip"), kw.get("predictor", True))


def test_round_trip_through_the_device_decoder(cases, batches, targeted):
    for mode in ("cv2", "4", "nopred"):
        files = batches[mode][0].files()
        frames = M.tiff.decode(files, device=DEV)
        for g, got in zip(cases[0][mode], frames):
            assert torch.equal(got, g[1]), g[0]
    files = E.encode([t[1] for t in targeted]).files()
    for (name, frame, _, _, _), got in zip(targeted, M.tiff.decode(files, device=DEV)):
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
    for rows in (0, 9, -1, [4, 4], [0], 2.0, "4", True):
        with pytest.raises(M.MafError, match="rows_per_strip"):
            E.encode([good], rows_per_strip=rows)
    with pytest.raises(M.MafError, match="rows_per_strip 5 is outside 1..h for file 1"):
        E.encode([good, good], rects=np.array([[0, 0, 0, 8, 8], [1, 0, 0, 8, 4]]), rows_per_strip=5)
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(1, 65536, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="65535"):
        E.encode([torch.zeros(65536, 1, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(M.MafError, match="65535 files"):
        E.encode([good], rects=np.tile(np.array([[0, 0, 0, 1, 1]]), (65536, 1)))
    with pytest.raises(M.MafError, match="8 MiB"):
        E.encode([torch.zeros(2048, 2048, 3, dtype=torch.uint8, device=DEV)], rows_per_strip=2048)
    with pytest.raises(M.MafError, match="uint8"):
        E.encode([good.float()])
    with pytest.raises(M.MafError, match="stride"):
        E.encode([torch.zeros(8, 3, 8, dtype=torch.uint8, device=DEV).permute(0, 2, 1)])
    with pytest.raises(M.MafError, match="no frames"):
        E.encode([])
