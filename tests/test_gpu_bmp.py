"""-m gpu: BMP decoding on the device (csrc/bmp_decode.hip, maf-yolo_amd/bmp.py) against the fixture pixels of tests/golden/bmp_cases.npz
(Pillow's decodes of the same files, or of their bmp_ref.rewrite where Pillow departs from the rule, stored BGR).  Bit-exact: torch.equal, no
tolerance.  No Pillow here.

* every case (1 bit at widths 1, 7, 8, 9, 31, 32, 33; 4 bit at 1, 2, 3, 7, 8, 9; 8 and 24 bit at 1 to 5; 24-bit rows of 48 and 36 bytes; 32 bit
  plain and with both mask sets; height 1; top-down; every header size; the OS/2 3-byte palette; short palettes with indices past them; a gray
  palette; a gap before the data; RLE8 and RLE4: runs of 1 and 255, absolute runs of 3, 4, 5, 254 and 255, deltas mid-row and at a row's end,
  an empty-row end of line, an early end of bitmap, data after it, a full image without one, a delta's operands, an absolute header and an
  absolute payload on a 128-byte fetch boundary, noise over many windows, a single colour, 1 x 1) decoded in one call, alone, and again on
  another stream with check=False;
* the planes tap equals the rule book's index plane, so a pixel mismatch points at its kernel;
* eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* each malformed file raises MafError naming the file and the bits tests/bmp_ref.py predicts; with check=False the other files of the call
  still decode exactly and the status words and index planes equal the rule book's (error reporting on input the kernel is built to bound:
  nothing here faults);
* frames.decode(webp=True, lossy=True, tiff=True, bmp=True) on a mixed list of JPEG, PNG, WebP, TIFF, BMP and MPO fixtures equals the decoders'
  own outputs, in order, and every BMP fixture through the router equals Pillow's pixels.
"""
import numpy as np
import pytest
import torch

import bmp_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import bmp as B

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("bmp_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call, with the taps (shared by the tests below; never modified)."""
    names, files, want, _ = cases
    taps = {}
    return B.decode(files, device=DEV, taps=taps), taps


@pytest.fixture(scope="module")
def malformed(cases):
    z = cases[3]
    names = [str(n) for n in z["bad_names"]]
    return names, [z["badfile_" + n].tobytes() for n in names], [int(z["badstatus_" + n]) for n in names]


def test_planes_tap_equals_the_rule_book(cases, batch):
    names, files, _, _ = cases
    taps = batch[1]
    assert taps["status"].dtype == torch.int32 and int(taps["status"].abs().sum()) == 0
    planes = taps["planes"].cpu().numpy()
    rle = [i for i, n in enumerate(names) if n.startswith("rle")]
    assert taps["rle"].tolist() == rle and int(taps["header"]["n_rle"]) == len(rle) >= 26
    for i in rle:
        want = R.decode_stages(files[i])[1]
        o = int(taps["images"][i]["plane_off"])
        assert np.array_equal(planes[o:o + want.size], want.reshape(-1)), names[i]


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
        got = B.decode([f], device=DEV)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = B.decode(files, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch[0]):
        assert torch.equal(got, b), n


def test_a_call_without_rle_files(cases, batch):
    """The RLE launch is skipped: the uncompressed files decode as in the batch."""
    names, files, want, _ = cases
    pick = [i for i, n in enumerate(names) if not n.startswith("rle")]
    taps = {}
    got = B.decode([files[i] for i in pick], device=DEV, taps=taps)
    assert int(taps["header"]["n_rle"]) == 0 and int(taps["header"]["planes_bytes"]) == 0
    for i, g in zip(pick, got):
        assert torch.equal(g, batch[0][i]), names[i]


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, _ = cases
    pick = [names.index("rle8_noise_70x50"), names.index("rle4_noise_70x50")]
    got = M.eval_batch([batch[0][i] for i in pick], img_size=160)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=160)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_malformed_files_raise_with_the_predicted_bits(cases, malformed, tmp_path):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    assert len(bad_names) >= 6 and {1, 2, 4} == set(bad_status)
    for n, f, st in zip(bad_names, bad_files, bad_status):
        assert R.decode_stages(f)[2] == st and st != 0, n            # the rule book, on the CPU, first
        p = tmp_path / (n + ".bmp")
        p.write_bytes(f)
        with pytest.raises(M.MafError, match=r"file 1 \(.*%s\.bmp\): .*\(status 0x%x\)" % (n, st)) as e:
            B.decode([files[3], str(p), files[7]], device=DEV)
        assert not isinstance(e.value, B.BmpUnsupported) and B.status_text(st) in str(e.value), n


def test_status_words_and_the_good_files_of_the_same_call(cases, malformed):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    good = [(5 * k + 1) % len(files) for k in range(len(bad_files) + 1)]
    mix = [files[good[0]]]
    for k, f in enumerate(bad_files):
        mix += [f, files[good[k + 1]]]
    taps = {}
    frames, status = B.decode(mix, device=DEV, check=False, taps=taps)
    st = status.tolist()
    assert st[0::2] == [0] * len(good) and st[1::2] == bad_status
    for k, i in enumerate(good):
        assert torch.equal(frames[2 * k].cpu(), want[i]), names[i]
    planes = taps["planes"].cpu().numpy()
    for k, n in enumerate(bad_names):                                 # the size the header names; the pixels up to the fault, zeros behind it
        info = B.parse(bad_files[k])
        assert tuple(frames[2 * k + 1].shape) == (info.height, info.width, 3), n
        bgr, plane, _ = R.decode_stages(bad_files[k])
        o = int(taps["images"][2 * k + 1]["plane_off"])
        assert np.array_equal(planes[o:o + plane.size], plane.reshape(-1)), n
        assert np.array_equal(frames[2 * k + 1].cpu().numpy(), bgr), n


def test_router_on_a_mixed_list(cases, batch, golden):
    names, files, want, z = cases
    jz, pz, wz, lz, tz = golden("jpeg_cases"), golden("png_cases"), golden("webp_cases"), golden("webp_lossy_cases"), golden("tiff_cases")
    jfiles = [jz["file_" + str(n)].tobytes() for n in jz["names"][:1]] + [z["mpofile_mpo_two_frames_420"].tobytes()]
    pfiles = [pz["file_" + str(n)].tobytes() for n in pz["names"][:1]]
    wfiles = [wz["file_" + str(n)].tobytes() for n in wz["names"][:1]] + [lz["file_" + str(n)].tobytes() for n in lz["names"][:1]]
    tfiles = [tz["file_" + str(n)].tobytes() for n in tz["names"][:1]]
    jframes, pframes, tframes = M.jpeg.decode(jfiles, device=DEV), M.png.decode(pfiles, device=DEV), M.tiff.decode(tfiles, device=DEV)
    wframes = [M.webp.decode(wfiles[:1], device=DEV)[0], M.webp_lossy.decode(wfiles[1:], device=DEV)[0]]
    a, b, c = names.index("rle8_noise_70x50"), names.index("bi1_w33"), names.index("bgr24_13x3_top_down")
    mix = [files[a], jfiles[0], wfiles[0], pfiles[0], files[b], jfiles[1], tfiles[0], wfiles[1], files[c]]
    expect = [batch[0][a], jframes[0], wframes[0], pframes[0], batch[0][b], jframes[1], tframes[0], wframes[1], batch[0][c]]
    got = M.frames.decode(mix, device=DEV, webp=True, lossy=True, tiff=True, bmp=True)
    assert len(got) == len(mix)
    for g, e in zip(got, expect):
        assert torch.equal(g, e)
    got, status = M.frames.decode(mix, device=DEV, check=False, webp=True, lossy=True, tiff=True, bmp=True)
    assert status.tolist() == [0] * len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))
    with pytest.raises(M.MafError, match="file 0: neither a JPEG nor a PNG signature"):
        M.frames.decode(mix, device=DEV, webp=True, lossy=True, tiff=True)
    # every fixture through the router, behind a JPEG: Pillow's pixels
    got = M.frames.decode([jfiles[0]] + files, device=DEV, bmp=True)
    assert torch.equal(got[0], jframes[0])
    for n, g, w in zip(names, got[1:], want):
        assert torch.equal(g.cpu(), w), n
