"""-m gpu: lossy WebP decoding on the device (csrc/vp8_decode.hip, maf-yolo_amd/webp_lossy.py) against the fixture pixels and planes of
tests/golden/webp_lossy_cases.npz (Pillow / libwebp decodes of the same files, stored BGR; WebPDecodeYUV's planes).  Bit-exact: torch.equal,
no tolerance.  No Pillow here.

* every case (sizes 1x1 ... 156x130 and 40x280, which has more macroblock rows than a band; qualities 1 ... 100; every intra mode, token and
  quantiser index; both loop filters, every sharpness class, filter deltas, 1 / 2 / 4 / 8 token partitions, segmentation on, off and absolute,
  with and without the skip probability, RGBA, a VP8X container with ICCP and EXIF) decoded in one call, alone, and again on another stream
  with check=False;
* the yuv tap equals y_ / u_ / v_<name> and the status words are all zero, so a pixel mismatch points at its stage; where the frame's filter
  level is 0 the recon tap equals them too;
* eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* each malformed file raises MafError naming the file and the bits tests/webp_lossy_ref.py predicts; with check=False the other files of the
  call still decode exactly, the bad file's frame is all zero and the status words equal the rule book's (error reporting on input the kernel
  is built to bound: nothing here faults);
* frames.decode(webp=True, lossy=True) on a mixed list of JPEG, PNG, lossless and lossy WebP fixtures equals the four decoders' own outputs,
  in order.
"""
import numpy as np
import pytest
import torch

import webp_lossy_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import webp as W, webp_lossy as WL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("webp_lossy_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call, with the taps (shared by the tests below; never modified)."""
    names, files, want, _ = cases
    taps = {}
    return WL.decode(files, device=DEV, taps=taps), taps


@pytest.fixture(scope="module")
def malformed(cases):
    z = cases[3]
    names = [str(n) for n in z["bad_names"]]
    return names, [z["badfile_" + n].tobytes() for n in names], [int(z["badstatus_" + n]) for n in names]


def test_yuv_tap_equals_the_fixture_planes(cases, batch):
    names, files, _, z = cases
    taps = batch[1]
    assert taps["status"].dtype == torch.int32 and int(taps["status"].abs().sum()) == 0
    yuv, recon = taps["yuv"].cpu(), taps["recon"].cpu()
    for n, f, im in zip(names, files, taps["images"]):
        for key, got, raw in zip("yuv", WL.plane_views(yuv, im), WL.plane_views(recon, im)):
            want = z[key + "_" + n]
            h, w = want.shape
            assert np.array_equal(got[:h, :w].numpy(), want), (n, key)
            if n == "t_level0":                                        # nothing is filtered: the planes before the loop filter are the same
                assert np.array_equal(raw[:h, :w].numpy(), want), (n, key, "recon")


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, _ = cases
    frames = batch[0]
    assert len(frames) == len(files) >= 60
    for n, got, w in zip(names, frames, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n


def test_each_case_alone_equals_the_batch(cases, batch):
    names, files, want, _ = cases
    for n, f, b, w in zip(names, files, batch[0], want):
        got = WL.decode([f], device=DEV)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = WL.decode(files, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch[0]):
        assert torch.equal(got, b), n


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, _ = cases
    pick = [names.index("mixed_64x65_q75_m4"), names.index("mixed_156x130_q30_m4")]
    got = M.eval_batch([batch[0][i] for i in pick], img_size=160)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=160)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_malformed_files_raise_with_the_predicted_bits(cases, malformed, tmp_path):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    assert len(bad_names) >= 5
    for n, f, st in zip(bad_names, bad_files, bad_status):
        assert R.decode_stages(f)[2] == st and st != 0, n            # the rule book, on the CPU, first
        p = tmp_path / (n + ".webp")
        p.write_bytes(f)
        with pytest.raises(M.MafError, match=r"file 1 \(.*%s\.webp\): .*\(status 0x%x\)" % (n, st)) as e:
            WL.decode([files[3], str(p), files[7]], device=DEV)
        assert not isinstance(e.value, W.WebpUnsupported) and WL.status_text(st) in str(e.value), n


def test_status_words_and_the_good_files_of_the_same_call(cases, malformed):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    good = [(3 * k + 1) % len(files) for k in range(len(bad_files) + 1)]
    mix = [files[good[0]]]
    for k, f in enumerate(bad_files):
        mix += [f, files[good[k + 1]]]
    frames, status = WL.decode(mix, device=DEV, check=False)
    st = status.tolist()
    assert st[0::2] == [0] * len(good) and st[1::2] == bad_status
    for k, i in enumerate(good):
        assert torch.equal(frames[2 * k].cpu(), want[i]), names[i]
    for k, n in enumerate(bad_names):                                 # an all-zero frame of the size the header names
        info = WL.parse(bad_files[k])
        got = frames[2 * k + 1]
        assert tuple(got.shape) == (info.height, info.width, 3) and not bool(got.any()), n


def test_router_on_a_mixed_list(cases, batch, golden):
    names, files, want, _ = cases
    jz, pz, wz = golden("jpeg_cases"), golden("png_cases"), golden("webp_cases")
    jfiles = [jz["file_" + str(n)].tobytes() for n in jz["names"][:2]]
    pfiles = [pz["file_" + str(n)].tobytes() for n in pz["names"][:2]]
    wfiles = [wz["file_" + str(n)].tobytes() for n in wz["names"][:2]]
    jframes, pframes, wframes = M.jpeg.decode(jfiles, device=DEV), M.png.decode(pfiles, device=DEV), M.webp.decode(wfiles, device=DEV)
    mix = [files[5], jfiles[0], wfiles[0], pfiles[0], files[16], jfiles[1], files[0], wfiles[1], pfiles[1]]
    expect = [batch[0][5], jframes[0], wframes[0], pframes[0], batch[0][16], jframes[1], batch[0][0], wframes[1], pframes[1]]
    got = M.frames.decode(mix, device=DEV, webp=True, lossy=True)
    assert len(got) == len(mix)
    for g, e in zip(got, expect):
        assert torch.equal(g, e)
    got, status = M.frames.decode(mix, device=DEV, check=False, webp=True, lossy=True)
    assert status.tolist() == [0] * len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))
    with pytest.raises(W.WebpUnsupported, match="a lossy file"):
        M.frames.decode(mix, device=DEV, webp=True)
