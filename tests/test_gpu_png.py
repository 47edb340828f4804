"""-m gpu: PNG decoding on the device (csrc/png_decode.hip, maf-yolo_amd/png.py) against the fixture pixels of tests/golden/png_cases.npz
(Pillow / libpng decodes of the same hand-written files, stored BGR).  Bit-exact: torch.equal, no tolerance.

* every case (sizes 1x1 ... 128x100, every colour type and bit depth, every filter type, stored / fixed / dynamic blocks, Z_RLE, Z_HUFFMAN_ONLY,
  memLevel 1, a full flush, 1- and 7-byte IDAT chunks, a match across 32 340 bytes) decoded in one call, alone, and again on another stream;
* the inflated-bytes tap equals inflated_<name> and the rows tap the rule book's, so a pixel mismatch points at its stage;
* a 480 x 640 file (925 KB of scanlines: the 32 KiB window wraps 28 times) written here from known pixels;
* eval_batch(decode(files)) equals eval_batch of the uploaded fixture frames;
* each malformed file raises MafError naming the file and the bits tests/png_ref.py predicts; with check=False the other files of the call still
  decode exactly and the status words equal the rule book's (error reporting on input the kernel is built to bound: nothing here faults);
* frames.decode on a mixed list of JPEG and PNG fixtures equals the two decoders' own outputs, in order.
"""
import numpy as np
import pytest
import torch

import png_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import png as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("png_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call, with the taps (shared by the tests below; never modified)."""
    names, files, want, _ = cases
    taps = {}
    return M.png.decode(files, device=DEV, taps=taps), taps


@pytest.fixture(scope="module")
def malformed(cases):
    z = cases[3]
    names = [str(n) for n in z["bad_names"]]
    return names, [z["badfile_" + n].tobytes() for n in names], [int(z["badstatus_" + n]) for n in names]


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, _ = cases
    frames = batch[0]
    assert len(frames) == len(files)
    for n, got, w in zip(names, frames, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n


def test_taps_equal_the_fixture_and_the_rule_book(cases, batch):
    names, files, _, z = cases
    taps = batch[1]
    inflated, rows = taps["inflated"].cpu().numpy(), taps["rows"].cpu().numpy()
    assert int(taps["status"].abs().sum()) == 0
    for n, f, im in zip(names, files, taps["images"]):
        o, size = int(im["inf_off"]), int(im["inflated_size"])
        assert np.array_equal(inflated[o:o + size], z["inflated_" + n]), (n, "inflated")
        h, rb = int(im["h"]), int(im["rowbytes"])
        want_rows = R.unfilter(z["inflated_" + n], h, rb, int(im["bpp"]))[0]
        o = int(im["rows_off"])
        assert np.array_equal(rows[o:o + h * rb].reshape(h, rb), want_rows), (n, "rows")


def test_each_case_alone_equals_the_batch(cases, batch):
    names, files, want, _ = cases
    for n, f, b, w in zip(names, files, batch[0], want):
        got = M.png.decode([f], device=DEV)[0]
        assert torch.equal(got, b) and torch.equal(got.cpu(), w), n


def test_second_call_on_another_stream(cases, batch):
    names, files, want, _ = cases
    s = torch.cuda.Stream(DEV)
    frames, status = M.png.decode(files, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and int(status.abs().sum()) == 0
    for n, got, b in zip(names, frames, batch[0]):
        assert torch.equal(got, b), n


def test_large_file_wraps_the_window(tmp_path):
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:480, 0:640]
    rgb = np.stack([(x // 3 + y) & 255, (x + y // 2) & 255, ((x // 16 + y // 16) & 1) * 180 + 20], -1).astype(np.uint8)
    rgb[:, 320:] += rng.integers(0, 16, (480, 320, 3), dtype=np.uint8)
    f, raw = R.encode(rgb.reshape(480, 640 * 3), 640, 8, 2, level=6)
    p = tmp_path / "large.png"
    p.write_bytes(f)
    taps = {}
    got = M.png.decode([str(p)], device=DEV, taps=taps)[0]
    assert tuple(got.shape) == (480, 640, 3)
    assert np.array_equal(taps["inflated"].cpu().numpy()[:raw.size], raw)
    assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])))


def test_frames_feed_eval_batch(cases, batch):
    names, files, want, _ = cases
    pick = [i for i, n in enumerate(names) if "64x48" in n or "128x100" in n]
    got = M.eval_batch([batch[0][i] for i in pick], img_size=128)
    ref = M.eval_batch([want[i].to(DEV) for i in pick], img_size=128)
    assert torch.equal(got[0], ref[0]) and got[1] == ref[1]


def test_malformed_files_raise_with_the_predicted_bits(cases, malformed, tmp_path):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    for n, f, st in zip(bad_names, bad_files, bad_status):
        assert R.decode_stages(f)[3] == st and st != 0, n          # the rule book, on the CPU, first
        p = tmp_path / (n + ".png")
        p.write_bytes(f)
        with pytest.raises(M.MafError, match=r"file 1 \(.*%s\.png\): .*\(status 0x%x\)" % (n, st)) as e:
            M.png.decode([files[4], str(p), files[5]], device=DEV)
        assert not isinstance(e.value, P.PngUnsupported) and P.status_text(st) in str(e.value), n


def test_status_words_and_the_good_files_of_the_same_call(cases, malformed):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    good = [4, 30, len(files) - 1, 12, 7]
    mix = [files[good[0]], bad_files[0], files[good[1]], bad_files[1], files[good[2]], bad_files[2], files[good[3]], bad_files[3], files[good[4]]]
    taps = {}
    frames, status = M.png.decode(mix, device=DEV, check=False, taps=taps)
    st = status.tolist()
    assert st[0::2] == [0] * 5 and st[1::2] == bad_status
    for k, i in enumerate(good):
        assert torch.equal(frames[2 * k].cpu(), want[i]), names[i]
    inflated = taps["inflated"].cpu().numpy()
    for k, f in enumerate(bad_files):                              # a zero-filled remainder, the pixels the rule book gives
        bgr, inf, _, _ = R.decode_stages(f)
        im = taps["images"][2 * k + 1]
        o = int(im["inf_off"])
        assert np.array_equal(inflated[o:o + inf.size], inf), bad_names[k]
        assert torch.equal(frames[2 * k + 1].cpu(), torch.from_numpy(bgr)), bad_names[k]


def test_router_on_a_mixed_list(cases, batch, golden):
    names, files, want, _ = cases
    jz = golden("jpeg_cases")
    jnames = [str(n) for n in jz["names"]][:3]
    jfiles = [jz["file_" + n].tobytes() for n in jnames]
    jframes = M.jpeg.decode(jfiles, device=DEV)
    mix = [files[5], jfiles[0], jfiles[1], files[20], jfiles[2], files[0]]
    expect = [batch[0][5], jframes[0], jframes[1], batch[0][20], jframes[2], batch[0][0]]
    got = M.frames.decode(mix, device=DEV)
    assert len(got) == len(mix)
    for g, e in zip(got, expect):
        assert torch.equal(g, e)
    got, status = M.frames.decode(mix, device=DEV, check=False)
    assert status.tolist() == [0] * len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))


def test_router_status_on_a_side_stream(cases, batch, malformed, golden):
    """check=False on a stream of the caller's: the merged status words are ordered behind the decoders' launches on THAT stream (the inflate
    launch is long), each file's word lands at its input position, and the host is not made to wait for them."""
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    jz = golden("jpeg_cases")
    jfiles = [jz["file_" + str(n)].tobytes() for n in jz["names"][:2]]
    big = files[names.index("stored_straddle_rgba16_128x100")]
    mix = [jfiles[0], big, bad_files[0], jfiles[1], files[5], bad_files[3], big]
    s = torch.cuda.Stream(DEV)
    frames, status = M.frames.decode(mix, device=DEV, stream=s, check=False)
    s.synchronize()
    assert status.dtype == torch.int32 and status.tolist() == [0, 0, bad_status[0], 0, 0, bad_status[3], 0]
    jframes = M.jpeg.decode(jfiles, device=DEV)
    assert torch.equal(frames[0], jframes[0]) and torch.equal(frames[3], jframes[1])
    assert torch.equal(frames[1], batch[0][names.index("stored_straddle_rgba16_128x100")]) and torch.equal(frames[4], batch[0][5])
