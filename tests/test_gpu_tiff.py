"""-m gpu: TIFF decoding on the device (csrc/tiff_decode.hip, maf-yolo_amd/tiff.py) against the fixture pixels of tests/golden/tiff_cases.npz
(Pillow / libtiff decodes of the same files, stored BGR).  Bit-exact: torch.equal, no tolerance.  No Pillow here.

* every case (LZW: a table that fills and walks every width with a Clear mid-strip, big-endian with predictor 2 and a short last strip, KwKwK,
  no EOI, trailing bytes, a Clear on the first and on the last code of a 64-code fetch, 1 x 1; PackBits: a run and a literal of 128, -128
  headers, a run across row ends, noise; Deflate: stored, fixed and dynamic blocks, both tag values, predictor 2, three strips; 1 / 4 / 8 bit
  with both gray photometrics, palettes, width 1, inline and offset strip tables) decoded in one call, alone, and again on another stream with
  check=False;
* the rows tap equals the rule book's decompressed rows, so a pixel mismatch points at its kernel;
* eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* each malformed file raises MafError naming the file and the bits tests/tiff_ref.py predicts; with check=False the other files of the call
  still decode exactly and the status words equal the rule book's (error reporting on input the kernel is built to bound: nothing here
  faults);
* frames.decode(webp=True, lossy=True, tiff=True) on a mixed list of JPEG, PNG, WebP and TIFF fixtures equals the decoders' own outputs, in
  order, and every TIFF fixture through the router equals Pillow's pixels.
"""
import numpy as np
import pytest
import torch

import tiff_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import tiff as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("tiff_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call, with the taps (shared by the tests below; never modified)."""
    names, files, want, _ = cases
    taps = {}
    return T.decode(files, device=DEV, taps=taps), taps


@pytest.fixture(scope="module")
def malformed(cases):
    z = cases[3]
    names = [str(n) for n in z["bad_names"]]
    return names, [z["badfile_" + n].tobytes() for n in names], [int(z["badstatus_" + n]) for n in names]


def test_rows_tap_equals_the_rule_book(cases, batch):
    names, files, _, _ = cases
    taps = batch[1]
    assert taps["status"].dtype == torch.int32 and int(taps["status"].abs().sum()) == 0
    rows = taps["rows"].cpu().numpy()
    assert int(taps["header"]["n_strips"]) == len(taps["strips"]) > len(files)
    for n, f, im in zip(names, files, taps["images"]):
        want = R.decode_stages(f)[1]
        o = int(im["rows_off"])
        assert np.array_equal(rows[o:o + want.size], want.reshape(-1)), n


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, _ = cases
    frames = batch[0]
    assert len(frames) == len(files) >= 40
    for n, got, w in zip(names, frames, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n


def test_each_case_alone_equals_the_batch(cases, batch):
    names, files, want, _ = cases
    for n, f, b, w in zip(names, files, batch[0], want):
        got = T.decode([f], device=DEV)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = T.decode(files, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch[0]):
        assert torch.equal(got, b), n


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, _ = cases
    pick = [names.index("lzw_rgb_noise_be_pred2_rps7"), names.index("pillow_tiff_lzw")]
    got = M.eval_batch([batch[0][i] for i in pick], img_size=160)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=160)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_malformed_files_raise_with_the_predicted_bits(cases, malformed, tmp_path):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    assert len(bad_names) >= 4
    for n, f, st in zip(bad_names, bad_files, bad_status):
        assert R.decode_stages(f)[2] == st and st != 0, n            # the rule book, on the CPU, first
        p = tmp_path / (n + ".tif")
        p.write_bytes(f)
        with pytest.raises(M.MafError, match=r"file 1 \(.*%s\.tif\): .*\(status 0x%x\)" % (n, st)) as e:
            T.decode([files[3], str(p), files[7]], device=DEV)
        assert not isinstance(e.value, T.TiffUnsupported) and T.status_text(st) in str(e.value), n


def test_status_words_and_the_good_files_of_the_same_call(cases, malformed):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    good = [(3 * k + 1) % len(files) for k in range(len(bad_files) + 1)]
    mix = [files[good[0]]]
    for k, f in enumerate(bad_files):
        mix += [f, files[good[k + 1]]]
    taps = {}
    frames, status = T.decode(mix, device=DEV, check=False, taps=taps)
    st = status.tolist()
    assert st[0::2] == [0] * len(good) and st[1::2] == bad_status
    for k, i in enumerate(good):
        assert torch.equal(frames[2 * k].cpu(), want[i]), names[i]
    rows = taps["rows"].cpu().numpy()
    for k, n in enumerate(bad_names):                                 # the size the IFD names; the rows up to the fault, zeros behind it
        info = T.parse(bad_files[k])
        assert tuple(frames[2 * k + 1].shape) == (info.height, info.width, 3), n
        ref = R.decode_stages(bad_files[k])[1].reshape(-1)
        o = int(taps["images"][2 * k + 1]["rows_off"])
        assert np.array_equal(rows[o:o + ref.size], ref), n


def test_router_on_a_mixed_list(cases, batch, golden):
    names, files, want, _ = cases
    jz, pz, wz, lz = golden("jpeg_cases"), golden("png_cases"), golden("webp_cases"), golden("webp_lossy_cases")
    jfiles = [jz["file_" + str(n)].tobytes() for n in jz["names"][:2]]
    pfiles = [pz["file_" + str(n)].tobytes() for n in pz["names"][:2]]
    wfiles = [wz["file_" + str(n)].tobytes() for n in wz["names"][:1]] + [lz["file_" + str(n)].tobytes() for n in lz["names"][:1]]
    jframes, pframes = M.jpeg.decode(jfiles, device=DEV), M.png.decode(pfiles, device=DEV)
    wframes = [M.webp.decode(wfiles[:1], device=DEV)[0], M.webp_lossy.decode(wfiles[1:], device=DEV)[0]]
    mix = [files[5], jfiles[0], wfiles[0], pfiles[0], files[16], jfiles[1], files[0], wfiles[1], pfiles[1]]
    expect = [batch[0][5], jframes[0], wframes[0], pframes[0], batch[0][16], jframes[1], batch[0][0], wframes[1], pframes[1]]
    got = M.frames.decode(mix, device=DEV, webp=True, lossy=True, tiff=True)
    assert len(got) == len(mix)
    for g, e in zip(got, expect):
        assert torch.equal(g, e)
    got, status = M.frames.decode(mix, device=DEV, check=False, webp=True, lossy=True, tiff=True)
    assert status.tolist() == [0] * len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))
    with pytest.raises(M.MafError, match="file 0: neither a JPEG nor a PNG signature"):
        M.frames.decode(mix, device=DEV, webp=True, lossy=True)
    # every fixture through the router, behind a JPEG: Pillow's pixels
    got = M.frames.decode([jfiles[0]] + files, device=DEV, webp=True, lossy=True, tiff=True)
    assert torch.equal(got[0], jframes[0])
    for n, g, w in zip(names, got[1:], want):
        assert torch.equal(g.cpu(), w), n
