"""-m gpu: baseline JPEG decoding on the device (csrc/jpeg_decode.hip, maf-yolo_amd/jpeg.py) against the fixture pixels of
tests/golden/jpeg_cases.npz (Pillow / libjpeg-turbo decodes of the same bytes, stored BGR).  Bit-exact: torch.equal, no tolerance.

* every case: sizes 1x1 ... 75x100, 4:4:4 / 4:2:2 / 4:2:0, quality 30 / 75 / 100, standard and optimised Huffman tables, restart intervals
  (the 17x33 4:4:4 one wraps the RSTn index), grayscale — decoded alone and all in one call, and again on another stream;
* the intermediate taps (coefficients, planes) equal tests/jpeg_ref.py, so a pixel mismatch points at its stage;
* the 480 x 640 case by the sha256 of the device frame's bytes;
* eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* a scan cut to half its length raises MafError naming the file; with check=False the other files of the call still decode exactly.
"""
import hashlib

import numpy as np
import pytest
import torch

import jpeg_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import jpeg as J

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("jpeg_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call (shared by the tests below; never modified)."""
    names, files, want, _ = cases
    return M.jpeg.decode(files, device=DEV)


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, _ = cases
    assert len(batch) == len(files)
    for n, got, w in zip(names, batch, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n


def test_each_case_alone_equals_the_batch(cases, batch):
    names, files, want, _ = cases
    for n, f, b, w in zip(names, files, batch, want):
        got = M.jpeg.decode([f], device=DEV)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = M.jpeg.decode(files, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch):
        assert torch.equal(got, b), n


@pytest.mark.parametrize("slots", [1, 8])
def test_lanes_packed_into_waves(cases, batch, monkeypatch, slots):
    """The host packs 1 lane per wave while the chip has free wave slots and up to 64 beyond; with fewer slots the same call takes the packed
    path (64 and 16 lanes per workgroup for the 94 lanes here, table sets padded to whole groups)."""
    names, files, want, _ = cases
    monkeypatch.setattr(J, "WAVE_SLOTS", slots)
    taps = {}
    frames = M.jpeg.decode(files, device=DEV, taps=taps)
    assert int(taps["header"]["group"]) == (64 if slots == 1 else 16)
    for n, got, b in zip(names, frames, batch):
        assert torch.equal(got, b), n


def test_taps_equal_the_restatement(cases):
    names, files, _, _ = cases
    pick = [i for i, n in enumerate(names) if n in ("grad_q75_7x9_s2", "noise_q30_opt_17x33_s1", "noise_q100_17x33_s0", "grad_q75_rst2_17x33_s2",
                                                     "gray_q75_17x33", "noise_q100_rstrow_75x100_s2")]
    assert len(pick) == 6
    taps = {}
    M.jpeg.decode([files[i] for i in pick], device=DEV, taps=taps)
    coef, planes = taps["coef"].cpu().numpy(), taps["planes"].cpu().numpy()
    for im, i in zip(taps["images"], pick):
        rc, status = R.coefficients(files[i])
        assert status == 0
        co, po = int(im["coef_off"]), int(im["plane_off"])
        q = J.parse(files[i])
        for c, comp in zip(rc, q.components):
            n = c.size
            assert np.array_equal(coef[co:co + n].reshape(c.shape), c), (names[i], "coefficients")
            assert np.array_equal(planes[po:po + n].reshape(8 * c.shape[0], 8 * c.shape[1]), R.idct_plane(c, q.qtables[comp.tq])), (names[i], "planes")
            co += n
            po += n


def test_large_case_sha256(cases):
    z = cases[3]
    got = M.jpeg.decode([z["large_file"].tobytes()], device=DEV)[0]
    assert tuple(got.shape) == (480, 640, 3)
    assert hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() == str(z["large_sha256"])


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, _ = cases
    pick = [i for i, n in enumerate(names) if "75x100" in n or "48x64" in n]
    got = M.eval_batch([batch[i] for i in pick], img_size=128)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=128)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_paths_and_orientation(cases, tmp_path):
    names, files, want, z = cases
    p = tmp_path / "a.jpg"
    p.write_bytes(files[5])
    assert torch.equal(M.jpeg.decode([str(p), files[6]], device=DEV)[0].cpu(), want[5])
    o6 = z["orientation6_file"].tobytes()
    with pytest.raises(J.JpegUnsupported, match="orientation 6"):
        M.jpeg.decode([files[0], o6], device=DEV)
    f = M.jpeg.decode([o6], device=DEV, ignore_orientation=True)[0]
    assert torch.equal(f.cpu(), torch.from_numpy(R.decode(o6))) and tuple(f.shape) == (16, 24, 3)
    with pytest.raises(J.JpegUnsupported, match="file 1.*progressive"):
        M.jpeg.decode([files[0], z["progressive_file"].tobytes()], device=DEV)
    with pytest.raises(M.MafError, match="HIP path only"):
        M.jpeg.decode([files[0]], device="cpu")


def test_status_word_of_a_truncated_scan(cases, tmp_path):
    names, files, want, _ = cases
    bad = []
    for n in ("noise_q30_opt_75x100_s2", "grad_q75_rst2_17x33_s0"):             # one lane per image, and one lane per restart interval
        d = files[names.index(n)]
        info = J.parse(d)
        bad.append(d[:info.scan[0] + (info.scan[1] - info.scan[0]) // 2] + b"\xff\xd9")
    p = tmp_path / "cut.jpg"
    p.write_bytes(bad[0])
    mix = [files[3], str(p), files[20], bad[1], files[40]]
    with pytest.raises(M.MafError, match=r"file 1 \(.*cut\.jpg\): a scan that ends early; file 3: a scan that ends early") as e:
        M.jpeg.decode(mix, device=DEV)
    assert not isinstance(e.value, J.JpegUnsupported)
    frames, status = M.jpeg.decode(mix, device=DEV, check=False)
    st = status.tolist()
    assert st[0] == 0 and st[2] == 0 and st[4] == 0 and st[1] & J.STATUS_SHORT_SCAN and st[3] & J.STATUS_SHORT_SCAN
    for k, i in ((0, 3), (2, 20), (4, 40)):
        assert torch.equal(frames[k].cpu(), want[i]), names[i]
