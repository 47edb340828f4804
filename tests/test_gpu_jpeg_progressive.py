"""-m gpu: progressive JPEG decoding on the device (csrc/jpeg_progressive.hip, maf-yolo_amd/jpeg.py with progressive=True) against the fixture
pixels of tests/golden/jpeg_progressive_cases.npz (Pillow / libjpeg-turbo decodes of the same bytes, stored BGR).  Bit-exact: torch.equal.

* every progressive case PLUS every baseline case of jpeg_cases.npz in one decode(..., progressive=True) call; each progressive case alone;
  again on another stream; with the lanes packed 64 and 16 to a wave;
* the coefficients after all rounds equal tests/jpeg_progressive_ref.py for a pick of cases (each subsampling, restarts, gray, the
  lengthened EOB run);
* the 480 x 640 case by the sha256 of the device frame's bytes; eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* short scans: the gray file (6 scans) cut in the middle of its 6th scan with EOI appended, and a colour file whose 6th scan loses its second
  half while scans 7 to 10 stay, in a mixed list: MafError naming the files; with check=False the neighbours still decode exactly.  (The
  same cut of a colour file would remove scans 7 to 10: an incomplete progression, which the parser refuses, tests/test_jpeg_progressive_host.py.)
"""
import hashlib

import numpy as np
import pytest
import torch

import jpeg_progressive_ref as P
import maf_yolo_amd as M
from maf_yolo_amd import jpeg as J

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    """Progressive cases first, then the baseline cases: names, file bytes, expected frames, number of progressive cases, the npz."""
    z, b = golden("jpeg_progressive_cases"), golden("jpeg_cases")
    pn, bn = [str(n) for n in z["names"]], [str(n) for n in b["names"]]
    names = ["prog_" + n for n in pn] + ["base_" + n for n in bn]
    files = [z["file_" + n].tobytes() for n in pn] + [b["file_" + n].tobytes() for n in bn]
    want = [torch.from_numpy(z["bgr_" + n]) for n in pn] + [torch.from_numpy(b["bgr_" + n]) for n in bn]
    return names, files, want, len(pn), z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call (shared by the tests below; never modified)."""
    names, files, want, _, _ = cases
    return M.jpeg.decode(files, device=DEV, progressive=True)


def test_progressive_and_baseline_cases_in_one_call_are_bit_exact(cases, batch):
    names, files, want, _, _ = cases
    assert len(batch) == len(files)
    for n, got, w in zip(names, batch, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n


def test_each_progressive_case_alone_equals_the_batch(cases, batch):
    names, files, want, n_prog, _ = cases
    for n, f, b, w in list(zip(names, files, batch, want))[:n_prog]:
        got = M.jpeg.decode([f], device=DEV, progressive=True)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = M.jpeg.decode(files, device=DEV, stream=s, check=False, progressive=True)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch):
        assert torch.equal(got, b), n


@pytest.mark.parametrize("slots", [1, 8])
def test_lanes_packed_into_waves(cases, batch, monkeypatch, slots):
    """With few wave slots the same call packs its lanes.  The scan lanes follow the baseline rule applied to the round with the most lanes
    (the Y scans: 161 lanes here, so 64 and 32 lanes per workgroup at 1 and 8 slots; the 94 baseline lanes 64 and 16 as in test_gpu_jpeg.py);
    every (image, scan) has Huffman tables of its own, so every table set is padded to a whole group."""
    names, files, want, _, _ = cases
    monkeypatch.setattr(J, "WAVE_SLOTS", slots)
    taps = {}
    frames = M.jpeg.decode(files, device=DEV, taps=taps, progressive=True)
    hdr, (scans, slanes, rounds) = taps["header"], taps["progressive"]
    most = max(int((slanes["image"][a:b] >= 0).sum()) for a, b in zip(rounds, rounds[1:]))
    expect = 64 if slots == 1 else 32
    assert most == 161 and int(hdr["sgroup"]) == expect and int(hdr["group"]) == (64 if slots == 1 else 16)
    assert all(int(r) % expect == 0 for r in rounds)
    for n, got, b in zip(names, frames, batch):
        assert torch.equal(got, b), n


def test_coefficients_after_all_rounds_equal_the_restatement(cases):
    names, files, _, _, _ = cases
    pick = [names.index("prog_" + n) for n in ("grad_q75_7x9_s2", "noise_q30_opt_17x33_s1", "noise_q100_17x33_s0", "noise_q100_17x33_s2",
                                               "grad_q75_rst2_17x33_s2", "grad_q75_rstrow_48x64_s1", "grad_q75_rst2_longeob_17x33_s0",
                                               "gray_q75_17x33", "grad_q75_1x1_s2")]
    taps = {}
    M.jpeg.decode([files[i] for i in pick], device=DEV, taps=taps, progressive=True)
    coef = taps["coef"].cpu().numpy()
    for im, i in zip(taps["images"], pick):
        rc, status = P.coefficients(files[i])
        assert status == 0
        co = int(im["coef_off"])
        for c in rc:
            assert np.array_equal(coef[co:co + c.size].reshape(c.shape), c), (names[i], "coefficients")
            co += c.size


def test_large_case_sha256(cases):
    z = cases[4]
    taps = {}
    got = M.jpeg.decode([z["large_file"].tobytes()], device=DEV, progressive=True, taps=taps)[0]
    assert tuple(got.shape) == (480, 640, 3) and int(taps["header"]["n_rounds"]) == 10
    assert hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() == str(z["large_sha256"])


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, n_prog, _ = cases
    pick = [i for i, n in enumerate(names[:n_prog]) if "75x100" in n or "48x64" in n]
    got = M.eval_batch([batch[i] for i in pick], img_size=128)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=128)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_status_word_of_a_short_scan(cases, tmp_path):
    names, files, want, n_prog, _ = cases
    g = files[names.index("prog_gray_q75_17x33")]
    r = J.parse(g, progressive=True).scans[5].range                      # the 6th and last scan of the gray file
    cut = g[:(r[0] + r[1]) // 2] + b"\xff\xd9"
    c = files[names.index("prog_noise_q30_opt_75x100_s2")]
    r = J.parse(c, progressive=True).scans[5].range                      # the 6th of 10: its second half goes, the scans behind it stay
    mid = c[:(r[0] + r[1]) // 2] + c[r[1]:]
    p = tmp_path / "cut.jpg"
    p.write_bytes(cut)
    keep = (3, n_prog + 20, 40)                                           # a progressive, a baseline and a progressive neighbour
    mix = [files[keep[0]], str(p), files[keep[1]], mid, files[keep[2]]]
    with pytest.raises(M.MafError, match=r"file 1 \(.*cut\.jpg\): a scan that ends early; file 3: a scan that ends early") as e:
        M.jpeg.decode(mix, device=DEV, progressive=True)
    assert not isinstance(e.value, J.JpegUnsupported)
    frames, status = M.jpeg.decode(mix, device=DEV, check=False, progressive=True)
    st = status.tolist()
    assert st[0] == 0 and st[2] == 0 and st[4] == 0 and st[1] & J.STATUS_SHORT_SCAN and st[3] & J.STATUS_SHORT_SCAN
    for k, i in zip((0, 2, 4), keep):
        assert torch.equal(frames[k].cpu(), want[i]), names[i]
    with pytest.raises(J.JpegUnsupported, match="file 1.*progressive"):  # and without the flag the call still refuses
        M.jpeg.decode([files[n_prog], files[0]], device=DEV)
