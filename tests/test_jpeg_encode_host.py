"""No GPU: the NumPy restatement of libjpeg's baseline encoder (tests/jpeg_encode_ref.py) against the files Pillow (libjpeg-turbo) wrote
into tests/golden/jpeg_encode_cases.npz, the host side of maf-yolo_amd/jpeg_encode.py (tables, headers, crop_rects, argument checks) and
the C-ABI's checks of the host blob.

* the reference's file equals the fixture's bytes for every case (and, where Pillow is installed, for 20 fresh random frames);
* the case set, seen through the reference's taps, still contains every rule's trigger (stuffing, ZRL, coefficient 63, DC category 11,
  AC size 10, dummy block columns and rows, an even 4:2:0 height that is no multiple of 16): trimming the fixture cannot drop one unnoticed;
* jpeg.parse accepts every fixture file and reports its size and sampling;
* crop_rects against rectangles worked out by hand.
"""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_encode_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import jpeg_encode as E
from maf_yolo_amd import lib

SS = {2: "4:2:0", 1: "4:4:4"}


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("jpeg_encode_cases")
    out = []
    for name, (h, w, hs, q) in zip((str(n) for n in z["names"]), z["meta"].tolist()):
        kind = name.split("_")[1]
        out.append((name, z["frame_%dx%d_%s" % (h, w, kind)], int(q), SS[hs], z["file_" + name].tobytes()))
    return out, z


@pytest.fixture(scope="module")
def reference(cases):
    """The reference's file and taps for every case (computed once; never modified)."""
    out = []
    for name, frame, q, ss, _ in cases[0]:
        taps = {}
        out.append((R.encode(frame, q, ss, taps=taps), taps))
    return out


def test_fixture_has_the_cases_the_issue_lists(cases):
    names = {c[0] for c in cases[0]}
    sizes = [(1, 1), (2, 2), (8, 8), (16, 16), (17, 19), (19, 17), (40, 25), (24, 40), (33, 47)]
    want = {"%dx%d_%s_%s_q%d" % (h, w, k, s, q) for h, w in sizes for k in ("random", "ramp", "saturated") for s in ("420", "444") for q in (30, 75, 95, 100)}
    assert names == want
    assert cases[1]["large_meta"].tolist() == [480, 640, 2, 95]


def test_reference_equals_libjpeg_for_every_case(cases, reference):
    for (name, _, _, _, want), (got, _) in zip(cases[0], reference):
        assert got == want, name


def test_reference_equals_libjpeg_for_the_large_frame(cases):
    assert R.encode(R.smooth_frame(480, 640), 95, "4:2:0") == cases[1]["large_file"].tobytes()


def test_case_set_triggers_every_rule(cases, reference):
    seen = dict.fromkeys(("stuffed", "zrl", "coef63", "dc11", "ac10", "dummy_col", "dummy_row", "even_h_420"), False)
    for (name, frame, q, ss, _), (_, t) in zip(cases[0], reference):
        h, w = frame.shape[:2]
        seen["stuffed"] |= bool((t["stream"] == 0xFF).any()) and len(t["scan"]) > len(t["stream"])
        coded, comp, real = t["coded"].astype(np.int64), t["coded_comp"], t["coded_real"]
        nz = coded != 0
        nz[:, 0] = True
        pos = np.where(nz, np.arange(64), 0)
        gaps = np.diff(np.maximum.accumulate(pos, axis=1), axis=1)            # a step of more than 16 positions between coded coefficients: a ZRL
        seen["zrl"] |= bool((gaps > 16).any())
        seen["coef63"] |= bool((coded[:, 63] != 0).any())
        for c in range(3):
            d = np.abs(np.diff(coded[comp == c, 0], prepend=0))
            seen["dc11"] |= bool((d >= 1024).any())
        seen["ac10"] |= bool((np.abs(coded[:, 1:]) >= 512).any())
        assert np.abs(coded[:, 1:]).max() < 1024 and np.abs(coded[:, 0]).max() <= 1024      # what the standard tables can code
        m = t["real"][0]
        seen["dummy_col"] |= bool((~m).all(0).any())
        seen["dummy_row"] |= bool((~m).all(1).any())
        seen["even_h_420"] |= ss == "4:2:0" and h % 2 == 0 and h % 16 != 0
        assert int(t["bits"].sum()) + (-int(t["bits"].sum()) % 8) == 8 * len(t["stream"])
        assert int(t["bits"].max()) <= E.BLOCK_BITS
        dummy_bits = {int(b) for b in t["bits"][~real]}
        assert dummy_bits <= {2 + 4}, name                                     # luma DC category 0 (2 bits) + luma EOB (4 bits)
    assert all(seen.values()), seen


def test_reference_equals_a_live_pillow_encode():
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    rng = np.random.default_rng(2024)
    for i in range(20):
        h, w = (int(v) for v in rng.integers(1, 49, 2))
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        q, ss = int(rng.integers(1, 101)), ("4:2:0", "4:4:4")[i % 2]
        buf = io.BytesIO()
        Image.fromarray(frame[..., ::-1]).save(buf, "JPEG", quality=q, subsampling=ss)
        assert R.encode(frame, q, ss) == buf.getvalue(), (h, w, q, ss)


def test_parse_accepts_every_fixture_file(cases):
    for name, frame, q, ss, data in cases[0]:
        info = M.jpeg.parse(data)
        assert (info.height, info.width) == frame.shape[:2], name
        assert [(c.h, c.v) for c in info.components] == [((2, 2) if ss == "4:2:0" else (1, 1)), (1, 1), (1, 1)], name
        assert info.restart_interval == 0 and info.orientation is None
        assert np.array_equal(info.qtables[0], E.quant_table(E.QUANT_LUMA, q)) and np.array_equal(info.qtables[1], E.quant_table(E.QUANT_CHROMA, q))
    info = M.jpeg.parse(cases[1]["large_file"].tobytes())
    assert (info.height, info.width) == (480, 640)


# ---------------------------------------------------------------- the module's host side

def test_module_tables_and_headers_equal_the_reference(cases):
    for mine, ref in zip(E.HUFFMAN, (R.DC_LUMA, R.DC_CHROMA, R.AC_LUMA, R.AC_CHROMA)):
        assert list(mine[0]) == list(ref[0]) and list(mine[1]) == list(ref[1])
        code, size = R.huff_codes(*ref)
        tab = E.huff_code_table(*mine).astype(np.int64)
        assert np.array_equal(tab >> 16, size) and np.array_equal(tab & 0xFFFF, code)
    for name, frame, q, ss, data in cases[0][::7]:
        h, w = frame.shape[:2]
        head = E.file_header(w, h, E.SAMPLING[ss], E.quant_table(E.QUANT_LUMA, q), E.quant_table(E.QUANT_CHROMA, q))
        assert data.startswith(head) and data[len(head) - 14:len(head) - 12] == b"\xff\xda", name


def test_crop_rects_by_hand():
    shape = (100, 200, 3)                                   # h 100, w 200
    det = np.array([
        # interior: centre (60, 50), wh (40, 20) -> wh * 1.02 + 10 = (50.8, 30.4); x 60 -+ 25.4 = 34.6 .. 85.4, y 50 -+ 15.2 = 34.8 .. 65.2 -> 34 34 85 65
        [40, 40, 80, 60],
        # corner below zero: centre (6, 4), wh (8, 4) -> (18.16, 14.08); x 6 -+ 9.08 = -3.08 .. 15.08, y 4 -+ 7.04 = -3.04 .. 11.04;
        # truncation toward zero gives -3 (floor would give -4), the clip 0 -> 0 0 15 11
        [2, 2, 10, 6],
        # past the right and bottom edge: centre (190, 95), wh (20, 10) -> (30.4, 20.2); x 174.8 .. 205.2, y 84.9 .. 105.1 -> 174 84 200 100
        [180, 90, 200, 100],
        # a centre ending in .5: centre (50.5, 30.5), wh (21, 11) -> (31.42, 21.22); x 34.79 .. 66.21, y 19.89 .. 41.11 -> 34 19 66 41
        [40, 25, 61, 36],
    ], np.float32)
    want = [[34, 34, 85, 65], [0, 0, 15, 11], [174, 84, 200, 100], [34, 19, 66, 41]]
    got = E.crop_rects(det, shape)
    assert got.dtype == np.int64 and got.tolist() == want
    assert E.crop_rects(torch.from_numpy(det), shape).tolist() == want
    assert E.crop_rects(np.concatenate([det, np.ones((4, 2), np.float32)], 1), shape).tolist() == want      # [x1 y1 x2 y2 conf cls] rows
    # square=True: the first box becomes 40 x 40 -> wh 50.8 both; y 50 -+ 25.4 = 24.6 .. 75.4 -> 34 24 85 75
    assert E.crop_rects(det[:1], shape, square=True).tolist() == [[34, 24, 85, 75]]
    # gain and pad are save_one_box's: wh (40, 20) * 1 + 0 -> the box itself
    assert E.crop_rects(det[:1], shape, gain=1.0, pad=0).tolist() == [[40, 40, 80, 60]]


def test_encode_refuses_cpu_tensors_and_bad_settings_before_any_device_work():
    f = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(M.MafError, match="no CPU fallback"):
        E.encode([f])
    for bad in (0, 101, 95.0, True):
        with pytest.raises(M.MafError, match="quality"):
            E.encode([f], quality=bad)
    for bad in ("4:2:2", "gray", 2):
        with pytest.raises(M.MafError, match="subsampling"):
            E.encode([f], subsampling=bad)
    with pytest.raises(M.MafError, match="no frames"):
        E.encode([])


def test_library_declares_the_symbols_and_struct_sizes():
    assert {"maf_jpeg_encode", "maf_jpeg_encode_struct_sizes"} <= set(lib.EXPORTS)
    sizes = (ctypes.c_int32 * 2)()
    lib.check(lib.load().maf_jpeg_encode_struct_sizes(sizes))
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize]


def _blob(edit=None, w=20, h=10, hs=2):
    """A valid host blob for one w x h file (a made-up frame pointer: the checks run before anything touches the device), after `edit`."""
    ql, qc = E.quant_table(E.QUANT_LUMA, 95), E.quant_table(E.QUANT_CHROMA, 95)
    head = np.frombuffer(E.file_header(w, h, hs, ql, qc), np.uint8)
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * hs))
    nb = mcux * mcuy * (hs * hs + 2)
    nc = -(-nb * E.BLOCK_BYTES // E.CHUNK)
    jobs = np.zeros(1, E.JOB_DT)
    jobs[0] = (4096, 3 * w, w, h, hs, mcux, mcuy, 0, nb, 0, nc, 0, len(head), 0)
    codes = np.concatenate([E.huff_code_table(*t) for t in E.HUFFMAN])
    quant = np.stack([ql, qc]).astype(np.uint16)
    hdr = np.zeros(1, E.HEADER_DT)
    hdr["n_files"], hdr["n_blocks"], hdr["n_chunks"] = 1, nb, nc
    hdr["heads_bytes"], hdr["out_bytes"] = len(head), len(head) + 2 + 2 * E.BLOCK_BYTES * nb
    parts = {"jobs": jobs, "codes": codes, "quant": quant, "head": head, "hdr": hdr}
    order = (("jobs", "jobs_off"), ("codes", "huff_off"), ("quant", "quant_off"), ("head", "heads_off"))
    off = 80
    for key, name in order:
        hdr[name] = off
        off = (off + parts[key].nbytes + 15) // 16 * 16
    hdr["total_bytes"] = off
    if edit:
        edit(parts)
    buf = np.zeros(off, np.uint8)
    for key, name in order:
        o = int(hdr[name][0])
        if 0 <= o and o + parts[key].nbytes <= buf.size:
            buf[o:o + parts[key].nbytes] = parts[key].reshape(-1).view(np.uint8)
    buf[:E.HEADER_DT.itemsize] = np.frombuffer(hdr.tobytes(), np.uint8)
    return buf


def _call(buf, null=None):
    args = [buf.ctypes.data] + [4096 * (i + 1) for i in range(10)] + [None]
    if null is not None:
        args[null] = None
    return lib.load().maf_jpeg_encode(*args)


@pytest.mark.parametrize("what, edit", [
    ("1 to 65535 files", lambda p: p["hdr"].__setitem__("n_files", 0)),
    ("outside the blob", lambda p: p["hdr"].__setitem__("heads_off", 1 << 20)),
    ("outside the blob", lambda p: p["hdr"].__setitem__("jobs_off", 88)),
    ("longer than 16 bits", lambda p: p["codes"].__setitem__(5, 17 << 16)),
    ("has no code", lambda p: p["codes"].__setitem__(512 + 0xF0, 0)),
    ("1..255", lambda p: p["quant"].__setitem__((0, 3), 0)),
    ("pointer is null", lambda p: p["jobs"].__setitem__("src", 0)),
    ("1 to 65535", lambda p: p["jobs"].__setitem__("w", 65536)),
    ("row pitch", lambda p: p["jobs"].__setitem__("pitch", 59)),
    ("sampling", lambda p: p["jobs"].__setitem__("hs", 3)),
    ("MCU counts", lambda p: p["jobs"].__setitem__("mcux", 3)),
    ("without gaps", lambda p: p["jobs"].__setitem__("block0", 6)),
    ("without gaps", lambda p: p["jobs"].__setitem__("n_blocks", 5)),
    ("worst case", lambda p: p["jobs"].__setitem__("n_chunks", 0)),
    ("header lies outside", lambda p: p["jobs"].__setitem__("head_len", 1 << 20)),
    ("differs from the jobs", lambda p: p["hdr"].__setitem__("n_blocks", 7)),
    ("smaller than the worst case", lambda p: p["hdr"].__setitem__("out_bytes", 1000)),
])
def test_c_abi_rejects_a_bad_blob_before_the_device(what, edit):
    rc = _call(_blob(edit))
    assert rc != 0
    assert what in lib.load().maf_last_error().decode()


def test_c_abi_rejects_null_and_misaligned_buffers():
    L = lib.load()
    assert _call(_blob(), null=3) != 0 and "null" in L.maf_last_error().decode()
    args = [_blob().ctypes.data, 4096 + 8] + [4096 * (i + 2) for i in range(9)] + [None]
    assert L.maf_jpeg_encode(*args) != 0 and "aligned" in L.maf_last_error().decode()
