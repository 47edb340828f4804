"""No GPU: the rule book of the TIFF encoder (tests/tiff_encode_ref.py) against its judge, Pillow / libtiff at cv2.imwrite's settings (LZW,
Predictor 2, RowsPerStrip); the fixtures; the hand-written binding.  Every comparison is ==.

* the rule book's strips equal the fixture's for every case and variant (the cv2 strip rule, 1, min(4, h) and h rows per strip, no predictor)
  and for the 480 x 640 frame; where Pillow with libtiff imports, they equal a fresh Image.save as well, for every fixture case and every
  targeted frame;
* the targeted frames (tiff_encode_ref.targeted_frames) have the property they were built for, asserted on the rule book's taps: the last data
  code at free = 511, 1023, 2047 (the EOI a bit wider), a strip that ends as the table fills, one and two table-full resets, a ratio checkpoint
  that only records, one that resets, a stream that ends on a byte boundary and one that needs padding, a 1 x 1 frame;
* the cv2 strip rule at w = 1, 2730, 2731, 65535; h not a multiple of rows_per_strip;
* tiff_ref.decode and Pillow read the rule book's files back to the exact pixels; the IFD is the eleven (ten) entries in ascending order;
* tiff_encode.py: the prototypes of include/mafyolo_tiff_encode.h, read by regex, equal the module's argtypes and restype; neither function is
  in lib.EXPORTS or mafyolo_hip.h; the struct sizes equal the built library's; the refusal texts; the worst-case bound holds on the fixtures and
  the targeted frames and noise comes within a stated fraction of it; a tampered blob is rejected on the host before any device pointer is used.
"""
import ctypes
import hashlib
import io
import os
import re

import numpy as np
import pytest

import tiff_encode_ref as R
import tiff_ref
from maf_yolo_amd import lib, staging, tiff_encode as E
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = (256, 257, 259, 262, 277, 278, 284, 317)


@pytest.fixture(scope="module")
def cases(golden):
    """(variant, frame, rows per strip, predictor, the fixture's strips, its tag values) per variant."""
    z = golden("tiff_encode_cases")
    out = []
    for variant in (str(v) for v in z["variants"]):
        name, mode = variant.rsplit("_", 1)
        frame = z["frame_" + name]
        tags = z["tags_" + variant].tolist()
        lens = z["lens_" + variant].tolist()
        blob = z["strips_" + variant].tobytes()
        ends = np.cumsum(lens).tolist()
        out.append((variant, frame, tags[5], mode != "nopred", [blob[e - n:e] for e, n in zip(ends, lens)], tags))
    return out, z


@pytest.fixture(scope="module")
def targeted():
    """name -> (frame, the rule book's taps, its file); built once, never modified."""
    out = {}
    for name, frame in R.targeted_frames().items():
        taps = {}
        out[name] = (frame, taps, R.encode(frame, taps=taps))
    return out


def libtiff_strips(bgr, rows_per_strip, predictor=True):
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    info = {278: int(rows_per_strip)}
    if predictor:
        info[317] = 2
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "TIFF", compression="tiff_lzw", tiffinfo=info)
    return R.file_strips(buf.getvalue())


def tag_values(tags):
    return [tags.get(t, [0])[0] for t in TAGS] + tags[258]


def test_rule_book_equals_the_fixture_on_every_case(cases):
    assert len(cases[0]) >= 120
    for variant, frame, rps, predictor, want, tags in cases[0]:
        data = R.encode(frame, rps, predictor)
        got_tags, got = R.file_strips(data)
        assert got == want, variant
        assert tag_values(got_tags) == tags, variant
    assert any(not c[3] for c in cases[0]) and any(len(c[4]) > 1 for c in cases[0])


def test_rule_book_equals_the_fixture_on_the_large_frame(cases):
    z = cases[1]
    data = R.encode(R.large_frame())
    tags, strips = R.file_strips(data)
    assert len(strips) == 120 and tags[278] == [4]
    assert [len(s) for s in strips] == z["large_lens"].tolist()
    assert hashlib.sha256(b"".join(strips)).hexdigest() == str(z["large_sha256"])
    assert tag_values(tags) == z["large_tags"].tolist()


def test_rule_book_equals_a_fresh_libtiff_on_the_fixture_cases(cases):
    for variant, frame, rps, predictor, want, tags in cases[0]:
        got_tags, got = libtiff_strips(frame, rps, predictor)
        assert got == want, variant                                                     # the fixture is what libtiff writes today
        assert tag_values(got_tags) == tags, variant


def test_rule_book_equals_a_fresh_libtiff_on_the_targeted_frames(targeted):
    for name, (frame, taps, data) in targeted.items():
        tags, want = libtiff_strips(frame, taps["rows_per_strip"])
        got_tags, got = R.file_strips(data)
        assert got == want, name
        assert tag_values(got_tags) == tag_values(tags), name


def test_targeted_frames_have_their_property(targeted):
    def strip(name):
        frame, taps, _ = targeted[name]
        assert len(taps["strips"]) == 1 and frame.shape[0] == 1, name               # one row, one strip
        return taps["strips"][0]
    for free in (511, 1023, 2047):
        t = strip("eoi_bump_%d" % free)
        assert t["free_at_end"] == free and t["clears"] == [0]
        assert t["widths"][-1] == t["widths"][-2] + 1 and t["codes"][-1] == R.EOI      # the EOI is a bit wider than the last data code
    t = strip("ends_as_table_fills")
    assert t["free_at_end"] == R.TABLE_FULL - 1 and t["codes"][-2:] == [R.CLEAR, R.EOI] and t["widths"][-2:] == [12, 9]
    assert len(t["clears"]) == 2 and not t["ratio_resets"]
    t = strip("one_table_full_reset")
    assert len(R.table_full_resets(t)) == 1 and not t["ratio_resets"] and t["codes"][-2] != R.CLEAR
    t = strip("two_table_full_resets")
    assert len(R.table_full_resets(t)) == 2 and not t["ratio_resets"] and t["codes"][-2] != R.CLEAR
    for c in R.table_full_resets(t):
        assert t["widths"][c] == 12 and t["widths"][c + 1] == 9                         # the Clear at the old width, then 9 bits again
    frame, taps, _ = targeted["ratio_records"]
    t = strip("ratio_records")
    assert frame.shape[1] >= 3334 and len(t["ratio_records"]) >= 1 and not t["ratio_resets"] and t["clears"] == [0]
    frame, taps, _ = targeted["ratio_resets"]
    t = strip("ratio_resets")
    assert frame.shape[1] == 10000 and len(t["ratio_resets"]) >= 1 and not R.table_full_resets(t)
    assert len(R.lzw(taps["raw"].tobytes())) < 5000                                     # 30 KB in, a few KB out
    assert strip("ends_on_a_byte")["bits"] % 8 == 0
    assert strip("needs_padding")["bits"] % 8 != 0
    frame, taps, data = targeted["one_pixel"]
    assert frame.shape == (1, 1, 3) and strip("one_pixel")["codes"][0] == R.CLEAR and len(strip("one_pixel")["codes"]) == 5


def test_ratio_reset_changes_the_stream():
    """Without the ratio rule the two-part strip would differ: the reset is not a no-op on the targeted frame."""
    t = {}
    R.lzw(R.two_part_row().tobytes(), t)
    at = t["ratio_resets"][0]
    assert t["codes"][at] == R.CLEAR and t["widths"][at + 1] == 9 and at + 1 < len(t["codes"]) - 1


def test_cv2_strip_rule():
    assert [R.cv2_rows_per_strip(w, 100) for w in (1, 2730, 2731, 65535)] == [100, 1, 1, 1]      # 8192 // 3 = 2730 rows, clamped to h; 8190 bytes; 8193 bytes
    assert R.cv2_rows_per_strip(1, 5000) == 2730 and R.cv2_rows_per_strip(640, 480) == 4 and R.cv2_rows_per_strip(1365, 9) == 2
    assert E.cv2_rows_per_strip(np.array([1, 2730, 2731, 65535, 1]), np.array([100, 100, 100, 100, 5000])).tolist() == [100, 1, 1, 1, 2730]


def test_height_that_is_no_multiple_of_rows_per_strip():
    frame = R.make_frame("photo", 37, 21, 5)
    taps = {}
    data = R.encode(frame, 4, taps=taps)
    tags, strips = R.file_strips(data)
    assert len(strips) == 10 and len(taps["raw"]) == 37 * 63
    assert strips[1] == R.lzw(R.differenced(frame[4:8]).tobytes())                     # a strip does not depend on the rest of the file
    assert strips[9] == R.lzw(R.differenced(frame[36:]).tobytes())                     # the last one holds one row
    _, want = libtiff_strips(frame, 4)
    assert strips == want
    assert np.array_equal(tiff_ref.decode(data), frame)


def test_readers_return_the_frames_and_the_layout_is_ours(cases, targeted):
    Image = pytest.importorskip("PIL.Image")
    todo = [(c[0], c[1], c[2], c[3]) for c in cases[0][::3]] + [(n, t[0], None, True) for n, t in targeted.items()]
    for name, frame, rps, predictor in todo:
        taps = {}
        data = R.encode(frame, rps, predictor, taps)
        assert np.array_equal(tiff_ref.decode(data), frame), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1], frame), name
        assert data[:4] == b"II*\0" and int.from_bytes(data[4:8], "little") == taps["ifd_at"] and taps["ifd_at"] % 2 == 0
        at = taps["ifd_at"]
        n = int.from_bytes(data[at:at + 2], "little")
        entries = [(int.from_bytes(data[e:e + 2], "little"), int.from_bytes(data[e + 2:e + 4], "little"), int.from_bytes(data[e + 4:e + 8], "little"))
                   for e in range(at + 2, at + 2 + 12 * n, 12)]
        want = [256, 257, 258, 259, 262, 273, 277, 278, 279, 284] + ([317] if predictor else [])
        assert [e[0] for e in entries] == want, name
        assert [e[1] for e in entries] == [R.LONG if t in (273, 279) else R.SHORT for t in want], name
        ns = len(taps["offsets"])
        assert [e[2] for e in entries] == [3 if t == 258 else ns if t in (273, 279) else 1 for t in want], name
        assert data[at + 2 + 12 * n:] == b"\0\0\0\0", name                              # next IFD 0, and the file ends there
        assert taps["offsets"][0] == 8 and np.array_equal(np.diff(taps["offsets"]), taps["lengths"][:-1]), name      # back to back, unpadded


# ---------------------------------------------------------------- the binding and the host side of the module

def test_header_prototypes_equal_the_binding():
    text = open(os.path.join(ROOT, "include", "mafyolo_tiff_encode.h")).read()
    protos = dict(re.findall(r"^int (maf_tiff_\w+)\(([^;]*)\);", text, re.M | re.S))
    assert set(protos) == set(E.PROTOTYPES)
    for name, args in protos.items():
        res, argtypes = E.PROTOTYPES[name]
        assert res is ctypes.c_int32
        params = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            assert "*" in p or "stream_t" in p, (name, p)                               # every parameter is a pointer or the stream handle
            assert t is ctypes.c_void_p or t == ctypes.POINTER(ctypes.c_int32)
    hip = open(os.path.join(ROOT, "include", "mafyolo_hip.h")).read()
    for name in E.PROTOTYPES:
        assert name not in lib.EXPORTS and name not in hip
    for const in ("CHUNK", "TABLE"):
        assert int(re.search(r"#define MAF_TIFF_ENC_%s (\d+)" % const, text).group(1)) == getattr(E, const)
    assert "#define MAF_TIFF_ENC_MAX_STRIP (1 << 23)" in text and E.MAX_STRIP == 1 << 23 == R.MAX_STRIP
    assert "#define MAF_TIFF_ENC_MAX_FILE ((int64_t)1 << 31)" in text and E.MAX_FILE == 1 << 31


def test_struct_sizes_equal_the_library():
    L = E._library()
    sizes = (ctypes.c_int32 * 3)()
    assert L.maf_tiff_encode_struct_sizes(sizes) == 0
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize, E.STRIP_DT.itemsize] == [56, 72, 16]


def test_worst_case_bound_holds_and_noise_comes_near_it(cases, targeted):
    """No strip of the fixtures or the targeted frames exceeds _worst_case_bytes / _worst_case_codes.  Noise: the rule book gives 11173 bytes
    for 8192 bytes of noise and 41005 for 30000, 1.36 to 1.37 bytes per byte, where the bound allows 1.5: a noise strip takes more than 0.9 of
    its bound (measured: 0.909 and 0.911)."""
    for frame, rps, predictor in [(c[1], c[2], c[3]) for c in cases[0]] + [(t[0], None, True) for t in targeted.values()]:
        taps = {}
        rows_per, strips = R.strips_of(frame, rps, predictor, taps)
        row = 3 * frame.shape[1]
        for k, (s, t) in enumerate(zip(strips, taps["strips"])):
            n = row * min(rows_per, frame.shape[0] - k * rows_per)
            assert len(s) <= E._worst_case_bytes(n) and len(t["codes"]) <= E._worst_case_codes(n)
    rng = np.random.default_rng(5)
    for n in (8192, 30000):
        z = R.lzw(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        assert 0.9 * E._worst_case_bytes(n) < len(z) <= E._worst_case_bytes(n)
    text = open(os.path.join(ROOT, "include", "mafyolo_tiff_encode.h")).read()
    assert "(int64_t)(n) + (int64_t)(n) / 3836 + (int64_t)(n) / 10000 + 2" in text and "(12 * MAF_TIFF_ENC_CODE_BOUND(n) + 7) / 8" in text
    assert E._worst_case_codes(7680) == 7680 + 2 + 0 + 2 and E._worst_case_bytes(7680) == (12 * 7684 + 7) // 8


def test_a_tampered_blob_is_rejected_on_the_host():
    L = E._library()
    w, h, rps = 5, 4, 2
    job = np.zeros(1, E.JOB_DT)
    job["src"], job["pitch"], job["w"], job["h"], job["rows_per_strip"], job["predictor"] = 4096, 15, w, h, rps, 1
    job["n_strips"], job["n_chunks"], job["code_slot"] = 2, 1, E._worst_case_codes(3 * w * rps)
    out_bytes = staging.align(8 + 2 * E._worst_case_bytes(3 * w * rps) + 1 + int(E._tail_bytes(np.int64(2), True)), 4)

    def call(jobs, **fields):
        hdr, off = staging.blob_layout(E.HEADER_DT, (("jobs_off", jobs),))
        hdr["n_files"], hdr["n_strips"], hdr["n_chunks"], hdr["total_bytes"] = 1, 2, 1, off
        hdr["raw_bytes"], hdr["code_elems"], hdr["out_bytes"] = staging.align(3 * w * h), 2 * int(job["code_slot"][0]), out_bytes
        for k, v in fields.items():
            hdr[k] = v
        buf = np.zeros(off, np.uint8)
        staging.write_blob(buf, hdr, (("jobs_off", jobs),))
        fake = 1 << 20                                                                  # never dereferenced: every call below fails validation first
        return L.maf_tiff_encode(buf.ctypes.data, *([fake] * 7), None)
    for field, value in (("w", 0), ("h", 70000), ("pitch", 14), ("predictor", 2), ("rows_per_strip", 0), ("rows_per_strip", 5), ("n_strips", 3),
                         ("n_chunks", 2), ("code_slot", 10), ("raw_off", 16), ("code_off", 2), ("src", 0), ("strip0", 1)):
        bad = job.copy()
        bad[field] = value
        assert call(bad) != 0, field
        with pytest.raises(MafError):
            lib.check(call(bad))
    for field, value in (("n_files", 0), ("n_strips", 3), ("n_chunks", 2), ("out_bytes", 12), ("out_bytes", out_bytes + 2), ("code_elems", 3), ("raw_bytes", 16),
                         ("jobs_off", 8), ("total_bytes", 16)):
        assert call(job, **{field: value}) != 0, field


def test_encode_refuses_cpu_frames_without_a_gpu():
    torch = pytest.importorskip("torch")
    with pytest.raises(MafError, match="no CPU fallback"):
        E.encode([torch.zeros(4, 4, 3, dtype=torch.uint8)])
    with pytest.raises(MafError, match="no frames"):
        E.encode([])


def test_refusal_texts(monkeypatch):
    """The refusals encode() makes itself, by name and before the library is called; the frames' own checks (no CPU fallback, empty, a side
    above 65535) are staging.frame_list's, worded in _FRAME_TEXT."""
    torch = pytest.importorskip("torch")

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(E, "_library", no_library)
    monkeypatch.setattr(E.staging, "frame_list", lambda frames, text: list(frames))     # host tensors stand in: nothing below touches their memory
    good = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for rows in (0, 9, -1, [4, 4], 2.0, "4", True):
        with pytest.raises(MafError, match="rows_per_strip"):
            E.encode([good], rows_per_strip=rows)
    with pytest.raises(MafError, match=r"rows_per_strip 9 is outside 1\.\.h for file 0 \(8 x 8\)"):
        E.encode([good], rows_per_strip=9)
    with pytest.raises(MafError, match="takes up to 65535 files per call"):
        E.encode([good], rects=np.tile(np.array([[0, 0, 0, 1, 1]]), (65536, 1)))
    wide = torch.zeros(1, 1, 3, dtype=torch.uint8).expand(2048, 2048, 3)
    with pytest.raises(MafError, match="strips of 12582912 bytes .2048 rows., fewer than 8 MiB are taken"):
        E.encode([wide], rows_per_strip=2048)
    huge = torch.zeros(1, 1, 3, dtype=torch.uint8).expand(40000, 20000, 3)
    with pytest.raises(MafError, match="fewer than 2 GiB are taken .BigTIFF is not done."):
        E.encode([huge])
    monkeypatch.setattr(E.staging, "MAX_BLOB", 64)                                      # a header and one job are 128 bytes; 65535 jobs never reach 2 GiB
    with pytest.raises(MafError, match="the job table of one call is limited to 2 GiB"):
        E.encode([good])
    monkeypatch.undo()
    assert "empty" in E._FRAME_TEXT["empty"] and "TIFF" in E._FRAME_TEXT["empty"] and "65535" in E._FRAME_TEXT["too_large"]
    assert "no CPU fallback" in E._FRAME_TEXT["cpu"] and all(t.startswith("tiff_encode.encode") for t in E._FRAME_TEXT.values())
