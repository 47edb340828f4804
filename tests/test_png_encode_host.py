"""No GPU: the rule book of the PNG encoder (tests/png_encode_ref.py) against its judge, the interpreter's zlib module at cv2.imwrite's settings
(zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)); the fixtures; the hand-written binding.  Every comparison is ==.

* the rule book's zlib stream equals zlib's on every fixture case, on 300 seeded random streams (mixed run lengths and alphabets) and for each of
  the five filters; the fixture files are what zlib writes today;
* the token list equals the run rule, written here a second time as a plain loop;
* Pillow and png_ref.decode read every fixture file back to the exact pixels; zlib.crc32 agrees with every chunk's CRC; the layout is signature,
  IHDR (8 bit, colour type 2), ONE IDAT, IEND and nothing else;
* the targeted streams (png_encode_ref.targeted_frames) have the property they were built for — asserted on the rule book's tokens and blocks —
  and equal zlib: 16382 / 16383 / 16384 / 2 x 16383 symbols (the empty last block), run remainders, a run across rows and across a block
  boundary, a constant frame (the second distance code is forced), no run at all (both are forced), tiny frames (fixed), noise (stored), a
  stored block behind a dynamic one off a byte boundary, Fibonacci frequencies that drive gen_bitlen past 15 bits, and a stream whose
  bit-length tree goes past 7 bits;
* frame_for_stream inverts the Sub filter; Adler-32 equals zlib.adler32;
* png_encode.py: the prototypes of include/mafyolo_png_encode.h, read by regex, equal the module's argtypes and restype; neither function is in
  lib.EXPORTS or mafyolo_hip.h; the struct sizes equal the built library's; the worst-case bound holds on the fixtures and the targeted streams
  and is tight on noise; a tampered blob is rejected on the host before any device pointer is used.
"""
import ctypes
import hashlib
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_encode_ref as R
import png_ref
from maf_yolo_amd import lib, png_encode as E, staging
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER_NAMES = {v: k for k, v in R.FILTERS.items()}


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("png_encode_cases")
    out = []
    for name, (h, w, ft) in zip((str(n) for n in z["names"]), z["meta"].tolist()):
        kind = name.split("_")[1]
        out.append((name, z["frame_%dx%d_%s" % (h, w, kind)], FILTER_NAMES[ft], z["file_" + name].tobytes()))
    return out, z


@pytest.fixture(scope="module")
def targeted():
    """name -> (frame, the rule book's taps, its file); built once, never modified."""
    out = {}
    for name, frame in R.targeted_frames().items():
        taps = {}
        out[name] = (frame, taps, R.encode(frame, "sub", taps))
    return out


def run_rule(raw):
    """The run rule of deflate_rle as a plain loop -> tokens (independent of png_encode_ref.tokenise, which is vectorised)."""
    raw = bytes(raw)
    out, i, n = [], 0, len(raw)
    while i < n:
        j = i
        while j < n and raw[j] == raw[i]:
            j += 1
        out.append(raw[i])
        r = j - i - 1
        while r >= 3:
            m = min(258, r)
            out.append(256 + m)
            r -= m
        out += [raw[i]] * r
        i = j
    return out


def random_stream(rng, i):
    n = int(rng.integers(1, 60000))
    alpha = int(rng.choice([1, 2, 3, 5, 17, 256]))
    mode = i % 4
    if mode == 0:
        return rng.integers(0, alpha, n, dtype=np.uint8)
    if mode == 1:
        runs = rng.geometric(rng.choice([0.5, 0.1, 0.01, 0.002]), n // 4 + 1)
        return np.repeat(rng.integers(0, alpha, runs.size, dtype=np.uint8), runs)[:n]
    if mode == 2:
        return np.concatenate([rng.integers(0, 256, n // 2, dtype=np.uint8), np.zeros(n, np.uint8)])
    runs = rng.integers(1, 600, n // 50 + 1)
    return np.repeat(rng.integers(0, alpha, runs.size, dtype=np.uint8), runs)


def test_the_judge_is_the_zlib_the_rules_were_written_for(cases):
    assert R.zlib_stream(b"abc")[:2] == b"\x78\x01"
    assert str(cases[1]["zlib_version"]) == "1.2.11"


def test_rule_book_equals_zlib_on_every_fixture_case(cases):
    assert len(cases[0]) >= 60
    assert {c[2] for c in cases[0]} == set(R.FILTERS)
    for name, frame, filt, want in cases[0]:
        taps = {}
        got = R.encode(frame, filt, taps)
        assert taps["zstream"] == R.zlib_stream(taps["raw"]), name
        assert got == want, name
        assert np.array_equal(taps["raw"], R.filtered(frame, filt))


def test_rule_book_equals_zlib_on_random_streams():
    rng = np.random.default_rng(0)
    for i in range(300):
        raw = random_stream(rng, i)
        assert R.deflate(raw) == R.zlib_stream(raw), i


def test_rule_book_equals_zlib_for_each_filter():
    for kind in ("noise", "flat", "ramp", "photo", "blocks"):
        frame = R.make_frame(kind, 41, 23, 3)
        streams = set()
        for filt in R.FILTERS:
            taps = {}
            R.encode(frame, filt, taps)
            assert taps["raw"][::1 + 3 * 23].tolist() == [R.FILTERS[filt]] * 41
            assert taps["zstream"] == R.zlib_stream(taps["raw"]), (kind, filt)
            streams.add(bytes(taps["raw"]))
        assert len(streams) == 5, kind


def test_tokens_equal_the_run_rule(cases, targeted):
    rng = np.random.default_rng(1)
    raws = [random_stream(rng, i)[:20000] for i in range(40)] + [t[1]["raw"] for t in targeted.values()] + [R.filtered(c[1], c[2]) for c in cases[0][::7]]
    raws += [np.zeros(n, np.uint8) for n in (1, 2, 3, 4, 5, 259, 260, 261, 262, 263, 517, 518, 519, 520, 521)]
    for raw in raws:
        assert R.tokenise(raw).tolist() == run_rule(raw)


def test_fixture_files_decode_to_the_exact_pixels_and_have_our_layout(cases):
    Image = pytest.importorskip("PIL.Image")
    for name, frame, _, data in cases[0]:
        assert np.array_equal(png_ref.decode(data), frame), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1], frame), name
        assert data[:8] == png_ref.SIGNATURE
        p, types = 8, []
        while p < len(data):
            n, = struct.unpack(">I", data[p:p + 4])
            typ, body, crc = data[p + 4:p + 8], data[p + 8:p + 8 + n], data[p + 8 + n:p + 12 + n]
            assert struct.unpack(">I", crc)[0] == zlib.crc32(typ + body), (name, typ)
            types.append(typ)
            if typ == b"IHDR":
                assert struct.unpack(">IIBBBBB", body) == (frame.shape[1], frame.shape[0], 8, 2, 0, 0, 0)
            if typ == b"IDAT":
                assert body[:2] == b"\x78\x01" and zlib.decompress(body) == bytes(R.filtered(frame, _filter_of(name)))
            p += 12 + n
        assert types == [b"IHDR", b"IDAT", b"IEND"] and p == len(data), name


def _filter_of(name):
    return name.rsplit("_", 1)[1]


def test_large_frame_sha256_is_what_zlib_writes(cases):
    frame = R.large_frame()
    taps = {}
    data = R.encode(frame, "sub", taps)
    assert taps["zstream"] == R.zlib_stream(taps["raw"])
    assert hashlib.sha256(data).hexdigest() == str(cases[1]["large_sha256"])
    kinds = {b[0] for b in taps["blocks"]}
    assert R.DYNAMIC in kinds and R.STORED in kinds and len(taps["blocks"]) > 30


def test_targeted_streams_equal_zlib(targeted):
    for name, (frame, taps, data) in targeted.items():
        assert np.array_equal(taps["raw"], R.filtered(frame, "sub")), name
        assert taps["zstream"] == R.zlib_stream(taps["raw"]), name
        assert np.array_equal(png_ref.decode(data), frame), name
        first = [b[1] for b in taps["blocks"]]
        assert first == [R.BLOCK_SYMBOLS * k for k in range(len(first))] and sum(b[2] for b in taps["blocks"]) == len(taps["tokens"])
        assert np.array_equal(np.diff(taps["bitoff"]), [b[3] for b in taps["blocks"][:-1]])


def test_targeted_streams_have_their_property(targeted):
    def blocks(name):
        return [(b[0], b[2]) for b in targeted[name][1]["blocks"]]

    def plans(name):
        t = targeted[name][1]
        return [R.block_plan(t["tokens"][b[1]:b[1] + b[2]]) for b in t["blocks"]]
    assert [n for _, n in blocks("symbols_16382")] == [16382]
    assert blocks("symbols_16383") == [(R.DYNAMIC, 16383), (R.FIXED, 0)]                 # the empty last block: fixed, end-of-block only
    assert targeted["symbols_16383"][1]["blocks"][1][3] == 10
    assert [n for _, n in blocks("symbols_16384")] == [16383, 1]
    assert [n for _, n in blocks("symbols_32766")] == [16383, 16383, 0]
    tk = targeted["run_across_blocks"][1]["tokens"]
    assert tk[16381] == 1 and tk[16382] == tk[16383] == 256 + 258                      # one run on both sides of the block boundary
    raw = targeted["run_across_blocks"][1]["raw"]
    assert (raw[16381:16381 + 3 * 121] == 1).all()                                      # ... and across rows, type bytes included
    raw = targeted["run_remainders"][1]["raw"]
    start = np.flatnonzero(np.concatenate([[True], raw[1:] != raw[:-1]]))
    runs = np.diff(np.concatenate([start, [raw.size]]))
    assert {int(r - 1) % 258 for r in runs if r - 1 >= 258} >= {0, 1, 2, 3} and {int(r - 1) for r in runs if r - 1 < 258} >= {0, 1, 2, 3, 4}
    p, = plans("flat")
    assert p["overflow"] == [0, 0, 0] and [n for n in p["dlen"] if n] == [1, 1] and (targeted["flat"][1]["tokens"] >= 256).sum() > 0
    p, = plans("no_runs")
    assert (targeted["no_runs"][1]["tokens"] < 256).all() and p["dlen"][:2] == [1, 1]
    assert blocks("tiny_1x1") == [(R.FIXED, 4)] and blocks("tiny_2x2")[0][0] == R.FIXED
    assert blocks("noise") == [(R.STORED, 64 * 193)]
    assert [t for t, _ in blocks("noise_two_blocks")] == [R.STORED, R.STORED]
    assert [t for t, _ in blocks("dynamic_then_stored")] == [R.DYNAMIC, R.STORED]
    assert (targeted["dynamic_then_stored"][1]["bitoff"][1] + 3) % 8 != 0              # the stored block pads: it starts off a byte boundary
    assert blocks("half_flat_half_noise")[0][0] == R.DYNAMIC
    p, = plans("fibonacci_16")
    assert p["overflow"][0] == 0 and max(p["llen"]) == 15                              # as deep as a code may be, without the repair
    for name in ("fibonacci_17", "fibonacci_18"):
        p, = plans(name)
        assert p["overflow"][0] > 0 and max(p["llen"]) == 15 and p["type"] == R.DYNAMIC, name
    p, = plans("bl_limit")
    assert p["overflow"][2] > 0 and max(p["bllen"]) == 7 and p["type"] == R.DYNAMIC


def test_frame_for_stream_inverts_the_sub_filter():
    rng = np.random.default_rng(2)
    s = rng.integers(0, 256, 6 * (1 + 3 * 11), dtype=np.uint8)
    s[::34] = 1
    assert np.array_equal(R.filtered(R.frame_for_stream(s, 11, 6), "sub"), s)
    with pytest.raises(AssertionError):
        R.frame_for_stream(np.zeros(34, np.uint8), 11, 1)


def test_adler32_equals_zlib():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5551, 5552, 5553, 70000):
        raw = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.adler32(raw) == zlib.adler32(bytes(raw))
        assert R.adler32(np.full(n, 255, np.uint8)) == zlib.adler32(b"\xff" * n)


# ---------------------------------------------------------------- the binding and the host side of the module

def test_header_prototypes_equal_the_binding():
    text = open(os.path.join(ROOT, "include", "mafyolo_png_encode.h")).read()
    protos = dict(re.findall(r"^int (maf_png_\w+)\(([^;]*)\);", text, re.M | re.S))
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
    for const in ("CHUNK", "BLOCK_SYMBOLS", "CODE_WORDS", "HEAD_WORDS", "FILE_BYTES"):
        assert int(re.search(r"#define MAF_PNG_ENC_%s (\d+)" % const, text).group(1)) == getattr(E, const)


def test_struct_sizes_equal_the_library():
    L = E._library()
    sizes = (ctypes.c_int32 * 3)()
    assert L.maf_png_encode_struct_sizes(sizes) == 0
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize, E.BLOCK_DT.itemsize] == [56, 72, 32]


def test_worst_case_bound_holds_and_is_tight_on_noise(cases, targeted):
    for raw, z in [(t[1]["raw"], t[1]["zstream"]) for t in targeted.values()] + [(R.filtered(c[1], c[2]), png_ref.walk(c[3])[2]) for c in cases[0]]:
        assert len(z) <= E._worst_case_bytes(len(raw))
    rng = np.random.default_rng(4)
    for n in (16383 * 3 - 1, 16383 * 3 + 7):                                            # stored blocks throughout: under 6 bytes a block from the bound
        raw = rng.integers(0, 256, n, dtype=np.uint8)
        z = R.zlib_stream(raw)
        assert 0 <= E._worst_case_bytes(n) - len(z) <= 6 + n // 16383 + 1


def test_a_tampered_blob_is_rejected_on_the_host():
    L = E._library()
    n_raw = 4 * (1 + 3 * 5)
    job = np.zeros(1, E.JOB_DT)
    packed = staging.align(E._worst_case_bytes(n_raw))
    job["src"], job["pitch"], job["w"], job["h"], job["filter"], job["n_raw"] = 4096, 15, 5, 4, 1, n_raw
    job["packed_bytes"], job["n_chunks"], job["n_blocks"] = packed, 1, 1

    def call(jobs, **fields):
        hdr, off = staging.blob_layout(E.HEADER_DT, (("jobs_off", jobs),))
        hdr["n_files"], hdr["n_chunks"], hdr["n_blocks"], hdr["total_bytes"] = 1, 1, 1, off
        hdr["raw_bytes"], hdr["packed_bytes"], hdr["out_bytes"] = staging.align(n_raw), packed, E.FILE_BYTES + E._worst_case_bytes(n_raw)
        for k, v in fields.items():
            hdr[k] = v
        buf = np.zeros(off, np.uint8)
        staging.write_blob(buf, hdr, (("jobs_off", jobs),))
        fake = 1 << 20                                                                  # never dereferenced: every call below fails validation first
        return L.maf_png_encode(buf.ctypes.data, *([fake] * 12), None)
    for field, value in (("w", 0), ("h", 70000), ("pitch", 14), ("filter", 5), ("n_raw", n_raw + 1), ("packed_bytes", packed - 16), ("n_chunks", 2),
                         ("n_blocks", 2), ("raw_off", 16), ("src", 0)):
        bad = job.copy()
        bad[field] = value
        assert call(bad) != 0, field
        with pytest.raises(MafError):
            lib.check(call(bad))
    for field, value in (("n_files", 0), ("n_chunks", 3), ("out_bytes", 10), ("jobs_off", 8), ("total_bytes", 16)):
        assert call(job, **{field: value}) != 0, field


def test_encode_refuses_cpu_frames_without_a_gpu():
    torch = pytest.importorskip("torch")
    with pytest.raises(MafError, match="no CPU fallback"):
        E.encode([torch.zeros(4, 4, 3, dtype=torch.uint8)])
    with pytest.raises(MafError, match="filter"):
        E.encode([torch.zeros(4, 4, 3, dtype=torch.uint8)], filter="adaptive")
