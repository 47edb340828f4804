"""No GPU: the rule book of the lossy WebP encoder (tests/webp_lossy_encode_ref.py) against the fixture and against its judges (Pillow and
webp_lossy_ref's decoder); the hand-written binding; the host side of maf-yolo_amd/webp_lossy_encode.py.

* the rule book writes every fixture file byte for byte and gives the fixture's taps; Pillow decodes each file to what webp_lossy_ref.decode_stages
  returns, and a decoder's unfiltered planes are the encoder's reconstruction;
* the cases have the property they were chosen for (padding, skips with use_skip = 1, 1 / 2 / 4 / 8 partitions with partition 0 owning two rows,
  cat6 tokens, the largest Y2 DC);
* the forward transforms invert within +-1 under webp_lossy_ref.idct / iwht; a stand-alone host program built from csrc/vp8_enc_rules.h gives
  the rule book's numbers on the fixture's blocks;
* the derived worst case: MB_BITS is webp_lossy_encode_ref.mb_worst_bits(), a bool never shifts more than bool_shifts says, the noise cases and
  a macroblock of the largest levels stay inside the bound, and the first partition inside its own;
* the closed-loop floor at base_q 0, 40 and 127 (derived next to the assertion);
* the prototypes of include/mafyolo_vp8_encode.h equal the module's binding, the struct sizes the library's; a tampered blob is rejected on the
  host; bad arguments raise before the library is called; frames.encode's handling of webp_lossy.
"""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

import png_encode_ref as P
import webp_lossy_encode_ref as R
import webp_lossy_ref as D
from webp_lossy_tables import AC_Q, COEFF_PROBA0
from maf_yolo_amd import frames as F, lib, staging, webp_lossy_encode as E
from maf_yolo_amd.lib import MafError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = (("y", "planes", 0), ("u", "planes", 1), ("v", "planes", 2), ("ry", "recon", 0), ("ru", "recon", 1), ("rv", "recon", 2))


def _args(a):
    base_q, level, lp = (int(v) for v in a)
    return base_q, None if level < 0 else level, lp


@pytest.fixture(scope="module")
def cases(golden):
    """[(name, frame, arguments, the fixture's file, the rule book's file and taps)], built once."""
    z = golden("webp_lossy_encode_cases")
    out = []
    for name, a in zip((str(n) for n in z["names"]), z["args"]):
        taps = {}
        data = R.encode(z["frame_" + name], *_args(a), taps=taps)
        out.append((name, z["frame_" + name], _args(a), z["file_" + name].tobytes(), data, taps))
    return out, z


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def test_rule_book_reproduces_the_fixture(cases):
    group, z = cases
    assert len(group) >= 15
    for name, _, _, want, got, taps in group:
        assert got == want, name
        for key, tap, i in TAPS:
            assert np.array_equal(taps[tap][i], z["%s_%s" % (key, name)]), (name, key)
        for key in ("ymodes", "uvmodes", "skips", "levels"):
            assert np.array_equal(taps[key], z["%s_%s" % (key, name)]), (name, key)
        assert taps["part_sizes"] == z["parts_" + name].tolist(), name


def test_every_file_is_judged_by_pillow_and_the_decoder(cases):
    for name, frame, (_, level, _), data, _, taps in cases[0]:
        h, w = frame.shape[:2]
        bgr, yuv, status = D.decode_stages(data)
        assert status == 0 and bgr.shape == frame.shape and np.array_equal(pillow_decode(data), bgr), name
        f, status, parts = D.describe(data)
        assert status == 0 and [b - a for a, b in parts] == taps["part_sizes"], name
        for got, want in zip(D.reconstruct(f), taps["recon"]):
            assert np.array_equal(got, want), name
        if level == 0:
            assert np.array_equal(yuv[0], taps["recon"][0][:h, :w]), name
        assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8 " and len(data) % 2 == 0 and int.from_bytes(data[4:8], "little") == len(data) - 8, name
        assert (f.xscale, f.yscale, f.colorspace, f.clamp, f.use_segment, f.use_lf_delta, f.sharpness, f.simple) == (0,) * 8 and f.dq == [0] * 5, name
        assert np.array_equal(f.proba, COEFF_PROBA0) and not any(mb["i4"] for mb in f.mbs), name


def test_cases_have_their_property(cases):
    t = {c[0]: c for c in cases[0]}
    assert [t[n][1].shape[:2] for n in ("1x1", "16x16", "17x16", "15x17", "33x47")] == [(1, 1), (16, 16), (17, 16), (15, 17), (33, 47)]
    flat = t["64x48_flat"][5]
    assert flat["frame"].use_skip == 1 and flat["skips"].sum() >= 3 and 0 < flat["frame"].skip_proba < 250
    assert [len(t["130x70_p%d" % lp][5]["part_sizes"]) for lp in (0, 1, 2, 3)] == [2, 3, 5, 9] and t["130x70_p3"][5]["frame"].mbh == 9
    assert t["1x1"][5]["frame"].log2_parts == 0 and t["33x47"][5]["frame"].log2_parts == 1 and t["48x48_noise_q0"][5]["frame"].log2_parts == 1
    assert np.abs(t["48x48_noise_q0"][5]["levels"]).max() >= 67                            # cat6
    assert t["48x48_noise_q127"][5]["frame"].base_q == 127 and t["48x48_noise_q127"][5]["frame"].level == 63
    white = t["32x32_white_mb"][5]
    assert np.abs(white["levels"]).max() == np.abs(white["levels"][:, 24, 0]).max() > 800 and abs(int(white["levels"][0, 24, 0])) > 800      # Y2 DCs: white against the 128 border, black against white
    assert {c[2][1] for c in cases[0]} == {None, 0}
    modes = np.concatenate([c[5]["ymodes"] for c in cases[0]])
    assert set(modes.tolist()) == {0, 1, 2, 3}
    assert set(np.concatenate([c[5]["uvmodes"] for c in cases[0]]).tolist()) == {0, 1, 2, 3}


def test_forward_transforms_invert_within_one():
    rng = np.random.default_rng(3)
    worst_dct = worst_wht = 0
    for _ in range(2000):
        res = rng.integers(-255, 256, (4, 4))
        worst_dct = max(worst_dct, int(np.abs(D.idct(R.fdct(res)) - res).max()))
        dc = rng.integers(-2040, 2041, 16).tolist()
        worst_wht = max(worst_wht, int(np.abs(np.array(D.iwht(R.fwht(dc))) - np.array(dc)).max()))
    assert worst_dct <= 1 and worst_wht <= 1
    assert R.fdct(np.full((4, 4), 9))[0] == 8 * 9 and R.fwht([8 * 9] * 16)[0] == 64 * 9      # twice an orthonormal transform's DC, twice over


PROGRAM = r"""
#include <cstdio>
#include "vp8_enc_rules.h"
int main() {
    int n;
    if (scanf("%d", &n) != 1) return 1;
    for (int i = 0; i < n; ++i) {
        int d[16], o[16];
        for (int k = 0; k < 16; ++k) if (scanf("%d", &d[k]) != 1) return 1;
        vp8e_fdct(d, o);
        for (int k = 0; k < 16; ++k) printf("%d ", o[k]);
        for (int k = 0; k < 16; ++k) printf("%d ", vp8e_fwht(o, k));
        for (int k = 0; k < 16; ++k) printf("%d ", vp8e_quantise(o[k], 4 + 7 * k));
        printf("%d %d %d\n", vp8e_luma(d[0] & 255, d[1] & 255, d[2] & 255), vp8e_chroma_u(d[3] & 1023, d[4] & 1023, d[5] & 1023),
               vp8e_chroma_v(d[3] & 1023, d[4] & 1023, d[5] & 1023));
    }
    return 0;
}
"""


def test_a_host_program_of_the_rules_header_equals_the_rule_book(cases, tmp_path):
    src = tmp_path / "rules.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "rules")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "maf-yolo_amd", "csrc"), str(src), "-o", exe])
    blocks = []
    for name in ("33x47", "48x48_noise_q0", "32x32_white_mb"):
        c = next(c for c in cases[0] if c[0] == name)
        src_y, rec_y = c[5]["planes"][0].astype(np.int32), c[5]["recon"][0].astype(np.int32)
        for y in range(0, src_y.shape[0], 4):
            for x in range(0, src_y.shape[1], 4):
                blocks.append(src_y[y:y + 4, x:x + 4] - np.roll(rec_y, 5, 1)[y:y + 4, x:x + 4])      # residuals of the fixture's samples, -255 .. 255
    text = "%d\n" % len(blocks) + "\n".join(" ".join(str(int(v)) for v in b.reshape(-1)) for b in blocks)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    assert len(blocks) >= 300
    for b, line in zip(blocks, out):
        got = [int(v) for v in line.split()]
        co = R.fdct(b)
        d = [int(v) for v in b.reshape(-1)]
        r4, g4, b4 = d[3] & 1023, d[4] & 1023, d[5] & 1023
        want = co + R.fwht(co) + [R.quantise(co[k], 4 + 7 * k) for k in range(16)] + [
            (16839 * (d[0] & 255) + 33059 * (d[1] & 255) + 6420 * (d[2] & 255) + (16 << 16) + (1 << 15)) >> 16,
            (-9719 * r4 - 19081 * g4 + 28800 * b4 + (128 << 18) + (1 << 17)) >> 18, (28800 * r4 - 24116 * g4 - 4684 * b4 + (128 << 18) + (1 << 17)) >> 18]
        assert got == want


# ---------------------------------------------------------------- the derived worst case

def _shifts(enc, prob, bit):
    before = enc.count + 8 * len(enc.out)
    enc.bit(prob, bit)
    return before - (enc.count + 8 * len(enc.out))


def test_the_worst_case_is_derived_and_holds(cases):
    assert E.MB_BITS == R.mb_worst_bits() and (E.HEADER_BOOLS, E.MODE_BOOLS, E.FLUSH_BYTES) == (R.HEADER_BOOLS, R.MODE_BOOLS, R.FLUSH_BYTES)
    assert max(R.bool_shifts(p, b) for p in range(256) for b in (0, 1)) == 7 and R.bool_shifts(128, 0) == R.bool_shifts(128, 1) == 1
    rng = np.random.default_rng(2)
    enc = D.BoolEncoder()
    for prob, bit in zip(rng.integers(1, 256, 20000).tolist(), rng.integers(0, 2, 20000).tolist()):
        assert _shifts(enc, prob, bit) <= R.bool_shifts(prob, bit)                       # no bool of a long random stream costs more than its bound
    # the partitions of every case, the noise cases among them, stay inside their bounds
    for name, _, _, data, _, taps in cases[0]:
        f = taps["frame"]
        n = 1 << f.log2_parts
        sizes = taps["part_sizes"]
        assert sizes[0] <= E._first_bound(f.mbw * f.mbh) < E.MAX_P0, name
        for p in range(n):
            assert sizes[1 + p] <= E._part_bound(f.mbw * len(range(p, f.mbh, n))), name
        assert len(data) <= E._worst_case_bytes(f.mbw, f.mbh, f.log2_parts)[1], name
    noise = next(c for c in cases[0] if c[0] == "48x48_noise_q0")
    assert sum(noise[5]["part_sizes"][1:]) * 8 > 0.25 * 9 * E.MB_BITS                        # ... and noise at base_q 0 comes within a factor of four
    # a macroblock of the largest levels, in every context
    f = D.Frame()
    for sign in (1, -1):
        for ctx in (0, 1):
            io = D.BoolEncoder()
            mb = dict(i4=0, levels=[[0 if (b < 16 and i == 0) else sign * 2047 for i in range(16)] for b in range(25)])
            D.walk_residuals(io, f, mb, [ctx] * 9, [ctx] * 9)
            assert 8 * (len(io.finish()) - E.FLUSH_BYTES) <= E.MB_BITS < 8 * 2600
    # the first partition: 1094 bools and at most 8 per macroblock; the largest file the host takes fits the frame tag's 19 bits
    assert E._first_bound(E.MAX_MBS) < E.MAX_P0 <= E._first_bound(E.MAX_MBS + 1)
    io = D.BoolEncoder()
    bools = []
    io_bit = io.bit
    io.bit = lambda p, b: bools.append(p) or io_bit(p, b)
    f.mbs = [dict(i4=0, ymode=1, uvmode=1, skip=0)]
    f.width = f.height = 16
    f.use_skip, f.skip_proba = 1, 200
    D.walk_header(io, f)
    D.walk_header_tail(io, f)
    assert len(bools) == E.HEADER_BOOLS
    D.walk_modes(io, f, f.mbs[0], [0] * 4, [0] * 4)
    assert len(bools) - E.HEADER_BOOLS == 7 <= E.MODE_BOOLS
    assert [E.quality_to_base_q(q) for q in (10, 50, 75, 90, 100)] == [75, 38, 26, 9, 0] == [R.quality_to_base_q(q) for q in (10, 50, 75, 90, 100)]
    assert E._AC_Q == AC_Q.tolist() and [E.default_filter_level(q) for q in (0, 30, 127)] == [1, 8, 63]


def test_closed_loop_floor():
    """The coefficients are twice an orthonormal transform's (a constant residual r gives DC 8 r against 4 r), so an error e in a coefficient is an
    error e / 2 in the orthonormal domain, and by Parseval the mean squared error of the samples is the mean of (e / 2)^2.  Round-to-nearest
    with step q keeps |e| <= q / 2: the root mean square error of a plane is at most q / 4, q the largest of the plane's steps.  The Y2 block is
    the same twice over: its coefficients are twice an orthonormal transform's of the luma DCs, so its steps count as q / 2.  Clipping to
    0 .. 255 only moves a sample towards its source.  On top comes the integer transforms' own rounding: max |idct(fdct(x)) - x| = 1 per sample
    and max |iwht(fwht(d)) - d| = 1 per luma DC, an eighth of a sample (test_forward_transforms_invert_within_one measures both), added to the
    root mean square by the triangle inequality.  Nothing here is fitted to what the encoder gives."""
    slack_dct, slack_wht = 1.0, 1.0 / 8
    frames = (P.make_frame("photo", 33, 47, seed=43), np.random.default_rng(11).integers(0, 256, (48, 48, 3), dtype=np.uint8))
    for base_q in (0, 40, 127):
        for frame in frames:
            taps = {}
            R.encode(frame, base_q, 0, 3, taps)
            assert np.abs(taps["levels"]).max() < 2047                                       # no level hit the clamp
            y1dc, y1ac, y2dc, y2ac, uvdc, uvac, _ = D.quantisers(taps["frame"])[0]
            steps = (max(y1ac, y2dc / 2, y2ac / 2), max(uvdc, uvac), max(uvdc, uvac))
            for k, (src, rec, q) in enumerate(zip(taps["planes"], taps["recon"], steps)):
                rms = float(np.sqrt(np.mean((src.astype(np.float64) - rec) ** 2)))
                bound = q / 4 + slack_dct + (slack_wht if k == 0 else 0)
                print("base_q %d plane %d: rms %.3f, bound %.3f" % (base_q, k, rms, bound))
                assert rms <= bound, (base_q, k, rms, bound)


# ---------------------------------------------------------------- the binding and the host side of the module

def test_header_prototypes_equal_the_binding():
    text = open(os.path.join(ROOT, "include", "mafyolo_vp8_encode.h")).read()
    protos = dict(re.findall(r"^int (maf_vp8_\w+)\(([^;]*)\);", text, re.M | re.S))
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
    for const in ("MAX_SIDE", "FILE_BYTES", "FRAME_BYTES", "HEADER_BOOLS", "MODE_BOOLS", "FLUSH_BYTES", "MB_BITS", "MB_LEVELS", "META_WORDS"):
        assert int(re.search(r"#define MAF_VP8_ENC_%s (\d+)" % const, text).group(1)) == getattr(E, const)
    assert "#define MAF_VP8_ENC_MAX_P0 (1 << 19)" in text and E.MAX_P0 == 1 << 19
    makefile = open(os.path.join(ROOT, "maf-yolo_amd", "csrc", "Makefile")).read()
    assert " vp8_encode.hip" in makefile and "mafyolo_vp8_encode.h" in makefile and " vp8_enc_rules.h" in makefile


def test_struct_sizes_equal_the_library():
    L = E._library()
    sizes = (ctypes.c_int32 * 2)()
    assert L.maf_vp8_encode_struct_sizes(sizes) == 0
    assert list(sizes) == [E.HEADER_DT.itemsize, E.JOB_DT.itemsize] == [64, 72]


def _blob(job_fields=None, header_fields=None):
    w, h = 40, 33
    mbw, mbh, lp = 3, 3, 1
    job = np.zeros(1, E.JOB_DT)
    parts, file_bytes = E._worst_case_bytes(mbw, mbh, lp)
    job["src"], job["pitch"], job["w"], job["h"], job["mbw"], job["mbh"], job["log2_parts"] = 4096, 3 * w, w, h, mbw, mbh, lp
    job["part_bytes"] = staging.align(parts)
    for k, v in (job_fields or {}).items():
        job[k] = v
    sections = (("jobs_off", job),)
    hdr, off = staging.blob_layout(E.HEADER_DT, sections)
    hdr["n_files"], hdr["base_q"], hdr["level"], hdr["max_chroma"], hdr["total_bytes"] = 1, 30, 8, 64 * mbw * mbh, off
    hdr["plane_bytes"], hdr["n_mbs"], hdr["part_bytes"], hdr["out_bytes"] = 384 * mbw * mbh, mbw * mbh, staging.align(parts), file_bytes
    for k, v in (header_fields or {}).items():
        hdr[k] = v
    buf = np.zeros(off, np.uint8)
    staging.write_blob(buf, hdr, sections)
    return buf


def test_a_tampered_blob_is_rejected_on_the_host():
    L = E._library()

    def call(buf):
        fake = 1 << 20                                                                  # never dereferenced: every call below fails validation first
        return L.maf_vp8_encode(buf.ctypes.data, *([fake] * 10), None)
    for field, value in (("w", 0), ("h", 16384), ("pitch", 119), ("mbw", 2), ("mbh", 4), ("log2_parts", 2), ("log2_parts", -1), ("log2_parts", 4), ("part_bytes", 1024),
                         ("part_off", 16), ("plane_off", 16), ("mb0", 1), ("src", 0)):
        rc = call(_blob(job_fields={field: value}))
        assert rc != 0, field
        with pytest.raises(MafError):
            lib.check(rc)
    for field, value in (("n_files", 0), ("base_q", 128), ("base_q", -1), ("level", 64), ("max_chroma", 64), ("n_mbs", 8), ("plane_bytes", 384), ("part_bytes", 16),
                         ("out_bytes", 100), ("jobs_off", 8), ("total_bytes", 16)):
        assert call(_blob(header_fields={field: value})) != 0, field
    wide = _blob(job_fields={"w": 16383, "h": 16383, "mbw": 1024, "mbh": 1024, "pitch": 3 * 16383})      # 2^20 macroblocks: the first partition's bound
    rc = call(wide)
    assert rc != 0
    with pytest.raises(MafError, match="19 bits"):
        lib.check(rc)


def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(E, "_library", lambda: pytest.fail("the library was called"))
    f = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(MafError, match="no CPU fallback"):
        E.encode([f])
    for kw, text in ((dict(quality=101), "quality is a number from 0 to 100"), (dict(quality=-1), "quality"), (dict(quality=None), "quality"),
                     (dict(base_q=128), "base_q is an int from 0 to 127"), (dict(base_q=3.0), "base_q"), (dict(base_q=True), "base_q"),
                     (dict(filter_level=64), "filter_level is an int from 0 to 63"), (dict(log2_parts=4), "log2_parts is an int from 0 to 3"),
                     (dict(log2_parts=-1), "log2_parts")):
        with pytest.raises(MafError, match=text):
            E.encode([f], **kw)
    with pytest.raises(MafError, match="no frames"):
        E.encode([])

    class OnDevice:
        """What staging.frame_list hands on for a CUDA frame: enough of a tensor for the size checks that follow it."""
        def __init__(self, h, w):
            self.shape = (h, w, 3)

        def stride(self, i):
            return (3 * self.shape[1], 3, 1)[i]

        def data_ptr(self):
            return 4096
    monkeypatch.setattr(staging, "frame_list", lambda frames, text: frames)
    for shape in ((1, 16384), (16384, 1)):
        with pytest.raises(MafError, match="a side is at most 16383"):
            E.encode([OnDevice(*shape)])
    with pytest.raises(MafError, match=r"65536 macroblocks: at most 65398 are taken .* 2\^19"):
        E.encode([OnDevice(4096, 4096)])
    with pytest.raises(MafError, match="up to 65535 files"):
        E.encode([OnDevice(4, 4)], rects=np.tile(np.array([[0, 0, 0, 4, 4]]), (65536, 1)))


def test_frames_encode_handles_webp_lossy(monkeypatch):
    torch = pytest.importorskip("torch")
    frames = [torch.zeros(4, 4, 3, dtype=torch.uint8)] * 2
    with pytest.raises(MafError, match="file 0 has suffix '.webp': no device encoder exists for it"):
        F.encode(frames, [".webp", ".png"])
    with pytest.raises(MafError, match=r"file 0 has suffix '.webp': no device encoder exists for it \(there is one for .jpg, .jpeg, .mpo, .png, .tif, .tiff, .bmp\)"):
        F.encode(frames, [".webp", ".png"])                                              # the refusal, word for word as before
    with pytest.raises(MafError, match="webp_lossless and webp_lossy are both given"):
        F.encode(frames, [".webp", ".png"], webp_lossless=True, webp_lossy=True)
    with pytest.raises(MafError, match="webp_lossless and webp_lossy are both given"):
        F.encode(frames, [".webp", ".png"], webp_lossless={}, webp_lossy=dict(quality=50))
    for bad in (False, 1, "yes", [("quality", 3)]):
        with pytest.raises(MafError, match="webp_lossy is None, True or a dict"):
            F.encode(frames, [".webp", ".png"], webp_lossy=bad)
    with pytest.raises(MafError, match="per-format arguments are jpeg=, png=, tiff= and bmp=, got webp"):
        F.encode(frames, [".webp", ".png"], webp_lossy=True, webp={})
    with pytest.raises(MafError, match="no device encoder exists for it"):
        F.encode(frames, [".webp", ".dng"], webp_lossy=True)
    with pytest.raises(MafError, match=r"webp_lossy_encode.encode runs on the HIP path only .* \[webp files of this call are inputs \[0\]\]"):
        F.encode(frames, [".WebP", ".png"], webp_lossy=True)
    seen = []

    class Batch:
        def __init__(self, n, tag):
            self.n, self.tag = n, tag

        def files(self):
            return [b"%s%d" % (self.tag, i) for i in range(self.n)]
    monkeypatch.setattr(F.webp_lossy_encode, "encode", lambda fr, **kw: seen.append((len(fr), kw)) or Batch(len(fr), b"v"))
    monkeypatch.setattr(F.webp_encode, "encode", lambda fr, **kw: pytest.fail("the lossless encoder was called"))
    monkeypatch.setitem(F.ENCODERS, "png", lambda fr, **kw: Batch(len(fr), b"p"))
    three = frames + frames[:1]
    assert F.encode(three, [".webp", ".png", ".webp"], webp_lossy=dict(quality=50)) == [b"v0", b"p0", b"v1"]
    assert F.encode(three, [".webp", ".png", ".webp"], webp_lossy=True) == [b"v0", b"p0", b"v1"]
    assert seen == [(2, {"quality": 50}), (2, {})]
    assert "webp" not in F.ENCODERS and ".webp" not in F.SUFFIX_FORMAT
