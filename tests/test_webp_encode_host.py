"""No GPU: the rule book of the lossless WebP encoder (tests/webp_encode_ref.py) against its judges, the decoders — libwebp through Pillow and
tests/webp_ref.py decode_stages — and against the fixture; the hand-written binding.  Every comparison is ==.

* the rule book writes every fixture file and every targeted file byte for byte; the targeted frames are the fixture's;
* Pillow and webp_ref.decode_stages read every fixture file and targeted file back to the exact pixels (status 0), decode_stages' ARGB before
  the inverse transforms are the rule book's residuals; webp.parse accepts the files; the layout is RIFF, WEBP, ONE VP8L chunk, a pad byte
  behind an odd payload, and both parities occur;
* the token list equals the run rule, written here a second time as a plain loop; the chosen modes equal a plain per-pixel loop over
  webp_ref.predict;
* the targeted frames have the property they were built for, asserted on the rule book's taps;
* the 480 x 640 frame: the rule book's file has the fixture's SHA-256, in well under a minute;
* all 14 modes are chosen somewhere in the fixture; the photo and smooth files are smaller than png_encode_ref's;
* webp_encode.py: the prototypes of include/mafyolo_webp_encode.h, read by regex, equal the module's argtypes and restype; neither function is in
  lib.EXPORTS or mafyolo_hip.h; the struct sizes equal the built library's; the worst-case bound holds on every file; a tampered blob is
  rejected on the host before any device pointer is used; bad arguments raise MafError before the library is called;
* frames.encode's handling of webp_lossless.
"""
import ctypes
import hashlib
import io
import os
import re
import struct
import time

import numpy as np
import pytest

import png_encode_ref as P
import webp_encode_ref as R
import webp_ref
from maf_yolo_amd import frames as F, lib, staging, webp, webp_encode as E
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    """[(name, frame, bits, the fixture's file, the rule book's taps and file)] for the fixture frames and for the targeted ones; built once."""
    z = golden("webp_encode_cases")
    out = []
    for names, bits, prefix in (("names", "bits", ""), ("targeted", "t_bits", "t_")):
        group = []
        for name, b in zip((str(n) for n in z[names]), z[bits].tolist()):
            frame, taps, stats = z[prefix + "frame_" + name], {}, []
            data = R.encode(frame, b, taps, stats)
            taps["stats"] = stats
            group.append((name, frame, b, z[prefix + "file_" + name].tobytes(), taps, data))
        out.append(group)
    return out[0], out[1], z


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def run_rule(px):
    """The run rule as a plain loop -> tokens (independent of webp_encode_ref.tokenise, which is vectorised)."""
    px = [int(v) for v in px]
    out, i, n = [], 0, len(px)
    while i < n:
        j = i
        while j < n and px[j] == px[i]:
            j += 1
        out.append(px[i] & 0xffffff)
        r = j - i - 1
        while r >= 3:
            m = min(4096, r)
            out.append(0x80000000 | m)
            r -= m
        out += [px[i] & 0xffffff] * r
        i = j
    return out


def modes_by_loop(frame, bits):
    """The mode rule pixel by pixel with webp_ref.predict -> (modes, residual pixels)."""
    h, w = frame.shape[:2]
    a = [int(v) for v in R.gather(frame)]
    bw, bh = webp_ref.subsample(w, bits), webp_ref.subsample(h, bits)
    cost = np.zeros((bw * bh, 14), np.int64)

    def sub(x, y):
        return sum(((x >> s & 255) - (y >> s & 255) & 255) << s for s in (0, 8, 16, 24))
    for y in range(1, h):
        for x in range(1, w):
            i = y * w + x
            for m in range(14):
                r = sub(a[i], webp_ref.predict(m, a[i - 1], a[i - w], a[i - w - 1], a[i - w + 1]))
                cost[(y >> bits) * bw + (x >> bits), m] += sum(min(r >> s & 255, 256 - (r >> s & 255)) for s in (0, 8, 16))
    modes = cost.argmin(1)
    res = []
    for i in range(w * h):
        y, x = divmod(i, w)
        pred = (0xff000000 if x == 0 else a[i - 1]) if y == 0 else a[i - w] if x == 0 else \
            webp_ref.predict(int(modes[(y >> bits) * bw + (x >> bits)]), a[i - 1], a[i - w], a[i - w - 1], a[i - w + 1])
        res.append(sub(a[i], pred))
    return modes, np.array(res, np.uint32)


def test_rule_book_equals_the_fixture_byte_for_byte(cases):
    assert len(cases[0]) >= 60 and len(cases[1]) >= 26
    for name, _, _, want, _, got in cases[0] + cases[1]:
        assert got == want, name


def test_targeted_frames_are_the_fixtures(cases):
    frames = R.targeted_frames()
    assert list(frames) == [c[0] for c in cases[1]]
    for name, frame, bits, _, _, _ in cases[1]:
        assert np.array_equal(frames[name][0], frame) and frames[name][1] == bits, name
    small = R.fixture_frames()
    assert list(small) == [c[0] for c in cases[0]]
    for name, frame, bits, _, _, _ in cases[0]:
        assert np.array_equal(small[name][0], frame) and small[name][1] == bits, name


def test_every_file_decodes_to_its_frame_and_has_our_layout(cases):
    parities = set()
    for name, frame, _, data, taps, _ in cases[0] + cases[1]:
        assert np.array_equal(pillow_decode(data), frame), name
        h, w = frame.shape[:2]
        bgr, argb, status = webp_ref.decode_stages(data)
        assert status == 0 and np.array_equal(bgr, frame), name
        assert np.array_equal(argb.reshape(-1), taps["images"][1]["px"]), name
        info = webp.parse(data)
        assert (info.width, info.height) == (w, h), name
        payload = taps["payload"]
        assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8L" and struct.unpack("<II", data[4:8] + data[16:20]) == (len(data) - 8, len(payload)), name
        assert data[20:20 + len(payload)] == payload and data[20 + len(payload):] == b"\0" * (len(payload) & 1), name
        assert payload[0] == 0x2f
        parities.add(len(payload) & 1)
    assert parities == {0, 1}


def test_tokens_equal_the_run_rule(cases):
    rng = np.random.default_rng(1)
    streams = [im["px"] for c in cases[1] for im in c[4]["images"]] + [im["px"] for c in cases[0][::5] for im in c[4]["images"]]
    streams += [np.zeros(n, np.uint32) for n in (1, 2, 3, 4, 5, 4096, 4097, 4098, 4099, 4100, 8192, 8193, 8196, 8197)]
    streams += [np.repeat(rng.integers(0, 3, 50).astype(np.uint32), rng.integers(1, 9000, 50)) for _ in range(4)]
    for px in streams:
        assert R.tokenise(px).tolist() == run_rule(px)


def test_modes_equal_a_plain_loop(cases):
    picked = [c for c in cases[0] if c[0] in ("17x19_photo_bits4", "33x47_noise_bits2", "33x47_ramp_bits3", "8x8_blocks_bits4")]
    picked += [c for c in cases[1] if c[0] in ("tr_edge", "clamping", "bits_2", "width_2", "below_green")]
    assert len(picked) == 9
    for name, frame, bits, _, taps, _ in picked:
        modes, res = modes_by_loop(frame, bits)
        assert np.array_equal(modes, taps["modes"]), name
        assert np.array_equal(res, taps["images"][1]["px"]), name


def test_targeted_frames_have_their_property(cases):
    t = {c[0]: c for c in cases[1]}

    def used(name, image, code):
        return np.flatnonzero(t[name][4]["images"][image]["hist"][code]).tolist()

    def copies(name):
        tok = t[name][4]["images"][1]["tokens"]
        return (tok[tok >= R.COPY] & 0xffff).tolist()
    assert [t[n][1].shape[:2] for n in ("tiny_1x1", "row_1x9", "column_9x1", "row_16384", "column_16384")] == [(1, 1), (1, 9), (9, 1), (1, 16384), (16384, 1)]
    assert t["width_2"][1].shape[1] == 2 and t["block_16x16"][4]["modes"].size == 1 and t["edge_17x33"][4]["modes"].size == 6 and t["edge_33x18"][4]["modes"].size == 6
    assert copies("runs_a") == [3, 4095, 4096] and copies("runs_b") == [4096, 4096] and copies("runs_c") == [4096, 4096, 3]
    tok = t["runs_a"][4]["images"][1]["tokens"].tolist()
    assert tok[:3] == [0x050607] * 3 and tok[5:7] == [0x050608, R.COPY | 3]               # r = 2: literals; r = 3: a copy
    tok = t["runs_b"][4]["images"][1]["tokens"].tolist()
    assert tok[:3] == [0x050607, R.COPY | 4096, 0x050607] and tok[5:10] == [0x050608, R.COPY | 4096, 0x050608, 0x050608, 0x010203]      # r = 4097, 4098
    assert t["runs_b"][1].shape[1] == 1
    flat = t["flat"][4]["images"][1]
    assert flat["tokens"].tolist() == [flat["tokens"][0], 0, R.COPY | 2686] and t["flat"][1].shape == (48, 56, 3)      # one run across 48 rows and 3 chunks
    for image in (0, 1):
        assert [len(used("black_1x3", image, c)) for c in range(5)] == [1, 1, 1, 1, 0]    # one symbol each; nothing uses the distance code
        assert all(not L.any() for L in t["black_1x3"][4]["images"][image]["lengths"])
    assert used("two_literals", 1, 0) == [4, 8] and used("two_literals", 1, 1) == [3, 9] and t["two_literals"][4]["images"][1]["head_bits"][:3] == [19, 19, 19]
    assert used("black_7x9", 1, 0) == [0, 256 + 11] and t["black_7x9"][4]["images"][1]["lengths"][0][[0, 267]].tolist() == [1, 1]
    assert t["black_7x9"][4]["images"][1]["head_bits"][0] > 19                            # a normal code: one of its two symbols is above 255
    assert t["fibonacci_16"][4]["stats"] == [] or all(s[0] == 0 for s in t["fibonacci_16"][4]["stats"])
    assert max(t["fibonacci_16"][4]["images"][1]["lengths"][0]) == 15
    for name in ("fibonacci_17", "fibonacci_18"):
        assert any(s[0] > 0 for s in t[name][4]["stats"]) and max(t[name][4]["images"][1]["lengths"][0]) == 15, name
    assert 4100 < t["fibonacci_17"][1].shape[1] < 4200
    assert any(s[1] > 0 for s in t["all_modes"][4]["stats"]) and any(s[1] > 0 for s in t["tr_edge"][4]["stats"])      # the 7-bit repair
    assert sorted(set(t["all_modes"][4]["modes"].tolist())) == list(range(14))
    edge = t["tr_edge"][4]["modes"].reshape(4, 3)[:, 2].tolist()
    assert t["tr_edge"][1].shape == (64, 35, 3) and set(edge) <= {3, 5, 9, 10} and len(set(edge)) >= 3, edge
    assert set(t["clamping"][4]["modes"].tolist()) >= {11, 12, 13}
    g = t["below_green"][1]
    assert (g[..., 1] > g[..., 0]).all() and (g[..., 1] > g[..., 2]).all() and set((R.gather(g) >> 16 & 255).tolist()) == {(10 - 200) % 256}
    assert t["bits_2"][2] == 2 and t["bits_2"][4]["modes"].size == 12 and t["bits_9"][2] == 9 and t["bits_9"][4]["modes"].size == 2


def test_large_frame_sha256_and_time(cases):
    t0 = time.time()
    data = R.encode(R.large_frame())
    assert time.time() - t0 < 30
    assert hashlib.sha256(data).hexdigest() == str(cases[2]["large_sha256"]) and len(data) == int(cases[2]["large_bytes"])
    assert np.array_equal(pillow_decode(data), R.large_frame())


def test_all_modes_are_chosen_and_smooth_content_beats_png(cases):
    modes = set()
    for c in cases[0] + cases[1]:
        modes |= set(c[4]["modes"].tolist())
    assert modes == set(range(14))
    checked = 0
    for name, frame, _, data, _, _ in cases[0]:
        if name.split("_")[1] in ("photo", "smooth") and frame.shape[0] >= 17:
            assert len(data) < len(P.encode(frame)), name
            checked += 1
    assert checked >= 6


# ---------------------------------------------------------------- the binding and the host side of the module

def test_header_prototypes_equal_the_binding():
    text = open(os.path.join(ROOT, "include", "mafyolo_webp_encode.h")).read()
    protos = dict(re.findall(r"^int (maf_webp_\w+)\(([^;]*)\);", text, re.M | re.S))
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
    for const in ("CHUNK", "COPY_CHUNK", "CODES", "CODE_WORDS", "HEAD_WORDS", "FILE_BYTES", "LEAD_BITS", "MAIN_BITS", "MAX_SIDE"):
        assert int(re.search(r"#define MAF_WEBP_ENC_%s (\d+)" % const, text).group(1)) == getattr(E, const)
    assert E.MAX_SIDE == webp.MAX_SIDE == R.MAX_SIDE and E.LEAD_BITS == R.LEAD_BITS


def test_struct_sizes_equal_the_library():
    L = E._library()
    sizes = (ctypes.c_int32 * 3)()
    assert L.maf_webp_encode_struct_sizes(sizes) == 0
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize, E.IMAGE_DT.itemsize] == [72, 64, 32]


def test_worst_case_bound_holds_and_descriptions_fit(cases):
    for name, frame, _, data, taps, _ in cases[0] + cases[1]:
        assert len(taps["payload"]) <= E._worst_case_bytes(frame.shape[0] * frame.shape[1], taps["modes"].size), name
        for im in taps["images"]:
            assert max(im["head_bits"]) <= 32 * E.HEAD_WORDS
    assert E._worst_case_bytes(1, 1) == (50 + 3 + 20480 + 90 + 7) // 8
    # the worst description: 280 lengths that no repeat token shortens, under a code-length code of 7 bits
    worst = 1 + 4 + 19 * 3 + 1 + 7 * 280
    assert worst <= 32 * E.HEAD_WORDS


def _blob(job_fields=None, image_fields=None, header_fields=None):
    w, h, bits = 5, 4, 4
    job = np.zeros(1, E.JOB_DT)
    packed = staging.align(E._worst_case_bytes(w * h, 1))
    job["src"], job["pitch"], job["w"], job["h"], job["bits"], job["bw"] = 4096, 15, w, h, bits, 1
    job["packed_bytes"], job["n_blocks"], job["n_copy"] = packed, 1, -(-packed // E.COPY_CHUNK)
    images = np.zeros(2, E.IMAGE_DT)
    images["n_px"], images["main"], images["alpha"], images["px_off"], images["chunk0"], images["n_chunks"] = [1, 20], [0, 1], [255, 0], [0, 4], [0, 1], [1, 1]
    for k, v in (job_fields or {}).items():
        job[k] = v
    for k, (i, v) in (image_fields or {}).items():
        images[k][i] = v
    sections = (("jobs_off", job), ("images_off", images))
    hdr, off = staging.blob_layout(E.HEADER_DT, sections)
    hdr["n_files"], hdr["n_images"], hdr["n_chunks"], hdr["n_blocks"], hdr["n_copy"], hdr["total_bytes"] = 1, 2, 2, 1, int(job["n_copy"][0]), off
    hdr["px_words"], hdr["packed_bytes"], hdr["out_bytes"] = 24, packed, E.FILE_BYTES + E._worst_case_bytes(w * h, 1) + 1
    for k, v in (header_fields or {}).items():
        hdr[k] = v
    buf = np.zeros(off, np.uint8)
    staging.write_blob(buf, hdr, sections)
    return buf


def test_a_tampered_blob_is_rejected_on_the_host():
    L = E._library()

    def call(buf, stream=None):
        fake = 1 << 20                                                                  # never dereferenced: every call below fails validation first
        return L.maf_webp_encode(buf.ctypes.data, *([fake] * 16), stream)
    for field, value in (("w", 0), ("h", 16385), ("pitch", 14), ("bits", 1), ("bits", 10), ("bw", 2), ("n_blocks", 2), ("packed_bytes", 16), ("n_copy", 9),
                         ("packed_off", 16), ("block0", 1), ("copy0", 1), ("src", 0)):
        rc = call(_blob(job_fields={field: value}))
        assert rc != 0, field
        with pytest.raises(MafError):
            lib.check(rc)
    for field, value in (("n_px", (1, 21)), ("n_px", (0, 2)), ("main", (0, 1)), ("alpha", (1, 255)), ("file", (1, 1)), ("px_off", (1, 8)), ("chunk0", (1, 0)),
                         ("n_chunks", (0, 2))):
        assert call(_blob(image_fields={field: value})) != 0, field
    for field, value in (("n_files", 0), ("n_images", 3), ("n_chunks", 3), ("n_copy", 0), ("out_bytes", 10), ("px_words", 23), ("jobs_off", 8), ("total_bytes", 16)):
        assert call(_blob(header_fields={field: value})) != 0, field


def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(E, "_library", lambda: pytest.fail("the library was called"))
    f = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(MafError, match="no CPU fallback"):
        E.encode([f])
    for bits in (1, 10):
        with pytest.raises(MafError, match="predictor_bits is an int from 2 to 9"):
            E.encode([f], bits)
    with pytest.raises(MafError):                                                        # the device test matches its own message: the CPU check comes first here
        E.encode([torch.zeros(0, 4, 3, dtype=torch.uint8)])
    with pytest.raises(MafError, match="no frames"):
        E.encode([])

    class OnDevice:
        """What staging.frame_list hands on for a CUDA frame: enough of a tensor for the size check that follows it."""
        def __init__(self, h, w):
            self.shape = (h, w, 3)

        def stride(self, i):
            return (3 * self.shape[1], 3, 1)[i]

        def data_ptr(self):
            return 4096
    monkeypatch.setattr(staging, "frame_list", lambda frames, text: frames)
    for shape in ((1, 16385), (16385, 1)):
        with pytest.raises(MafError, match="a side is at most 16384"):
            E.encode([OnDevice(*shape)])


def test_frames_encode_handles_webp_lossless(monkeypatch):
    torch = pytest.importorskip("torch")
    frames = [torch.zeros(4, 4, 3, dtype=torch.uint8)] * 2
    with pytest.raises(MafError, match="file 0 has suffix '.webp': no device encoder exists for it"):
        F.encode(frames, [".webp", ".png"])
    with pytest.raises(MafError, match="per-format arguments are jpeg=, png=, tiff= and bmp=, got webp"):
        F.encode(frames, [".webp", ".png"], webp={})
    with pytest.raises(MafError, match="per-format arguments are"):
        F.encode(frames, [".webp", ".png"], webp_lossless=True, webp={})
    for bad in (False, 1, "yes", [("predictor_bits", 3)]):
        with pytest.raises(MafError, match="webp_lossless is None, True or a dict"):
            F.encode(frames, [".webp", ".png"], webp_lossless=bad)
    with pytest.raises(MafError, match="no device encoder exists for it"):
        F.encode(frames, [".webp", ".dng"], webp_lossless=True)
    with pytest.raises(MafError, match=r"webp_encode.encode runs on the HIP path only .* \[webp files of this call are inputs \[0\]\]"):
        F.encode(frames, [".WebP", ".png"], webp_lossless=True)
    seen = []

    class Batch:
        def __init__(self, n, tag):
            self.n, self.tag = n, tag

        def files(self):
            return [b"%s%d" % (self.tag, i) for i in range(self.n)]
    monkeypatch.setattr(F.webp_encode, "encode", lambda fr, **kw: seen.append((len(fr), kw)) or Batch(len(fr), b"w"))
    monkeypatch.setitem(F.ENCODERS, "png", lambda fr, **kw: Batch(len(fr), b"p"))
    three = frames + frames[:1]
    assert F.encode(three, [".webp", ".png", ".webp"], webp_lossless=dict(predictor_bits=3)) == [b"w0", b"p0", b"w1"]
    assert F.encode(three, [".webp", ".png", ".webp"], webp_lossless=True) == [b"w0", b"p0", b"w1"]
    assert seen == [(2, {"predictor_bits": 3}), (2, {})]
    assert "webp" not in F.ENCODERS and ".webp" not in F.SUFFIX_FORMAT
