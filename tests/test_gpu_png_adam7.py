"""-m gpu: Adam7 PNG decoding on the device (png.decode(..., interlaced=True), csrc/png_decode.hip) against the fixture pixels of
tests/golden/png_adam7_cases.npz (Pillow / libpng decodes of hand-assembled files, stored BGR).  Bit-exact: torch.equal, no tolerance.

* every case (1x1 where only pass 1 exists, 1x9, 9x1, 2x2, 3x5, 5x3, 8x8, 9x17, 17x33, 37x131 whose pass 7 has 65 rows; every colour type and bit
  depth, tRNS on the palette files; filter types cycled by (row + pass) % 5; 5-byte IDAT chunks) decoded in one call and alone;
* the inflated-bytes tap equals inflated_<name> and the rows tap the rule book's sub-images back to back, so a mismatch points at its stage;
* one call that alternates interlaced and plain files: the plain frames equal those of a plain-only call;
* each malformed file raises MafError with the bits tests/png_adam7_ref.py predicts; with check=False the other files of the call still decode
  exactly and the status words and pixels equal the rule book's (error reporting on input the kernels are built to bound: nothing here faults);
* frames.decode(..., interlaced=True) on JPEG, plain and Adam7 files equals the decoders' own outputs, in order.
"""
import numpy as np
import pytest
import torch

import png_adam7_ref as A
import maf_yolo_amd as M
from maf_yolo_amd import png as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_CASES, N_MALFORMED = 37, 4          # the counts tools/make_golden_png_adam7.py wrote: no case can drop out silently


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("png_adam7_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z


@pytest.fixture(scope="module")
def batch(cases):
    """All cases decoded in ONE call, with the taps (shared by the tests below; never modified)."""
    taps = {}
    return M.png.decode(cases[1], device=DEV, taps=taps, interlaced=True), taps


@pytest.fixture(scope="module")
def malformed(cases):
    z = cases[3]
    names = [str(n) for n in z["bad_names"]]
    return names, [z["badfile_" + n].tobytes() for n in names], [int(z["badstatus_" + n]) for n in names]


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, _ = cases
    frames = batch[0]
    assert len(names) == len(frames) == N_CASES
    done = 0
    for n, got, w in zip(names, frames, want):
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape), n
        assert torch.equal(got.cpu(), w), n
        done += 1
    assert done == N_CASES and int(batch[1]["status"].abs().sum()) == 0


def test_taps_equal_the_fixture_and_the_rule_book(cases, batch):
    names, files, _, z = cases
    taps = batch[1]
    inflated, rows = taps["inflated"].cpu().numpy(), taps["rows"].cpu().numpy()
    assert taps["images"]["interlace"].tolist() == [1] * N_CASES
    for n, f, im in zip(names, files, taps["images"]):
        o, size = int(im["inf_off"]), int(im["inflated_size"])
        assert size == z["inflated_" + n].size and np.array_equal(inflated[o:o + size], z["inflated_" + n]), (n, "inflated")
        flat = A.decode_stages(f)[2]
        o = int(im["rows_off"])
        assert np.array_equal(rows[o:o + flat.size], flat), (n, "rows")


def test_each_case_alone_equals_the_batch(cases, batch):
    names, files, want, _ = cases
    done = 0
    for n, f, b, w in zip(names, files, batch[0], want):
        got, status = M.png.decode([f], device=DEV, check=False, interlaced=True)
        assert status.tolist() == [0] and torch.equal(got[0], b) and torch.equal(got[0].cpu(), w), n
        done += 1
    assert done == N_CASES


def test_interlaced_and_plain_files_alternate_in_one_call(cases, batch, golden):
    names, files, want, _ = cases
    pz = golden("png_cases")
    pnames = [n for n in (str(n) for n in pz["names"]) if "17x33" in n or "3x5" in n or "1x1" in n]
    pfiles = [pz["file_" + n].tobytes() for n in pnames]
    assert len(pnames) >= 20
    plain_only = M.png.decode(pfiles, device=DEV)                      # without the flag: the call of the parent commit
    k = min(len(pfiles), len(files))
    mix = [f for pair in zip(files[:k], pfiles[:k]) for f in pair]
    taps = {}
    got = M.png.decode(mix, device=DEV, interlaced=True, taps=taps)
    assert taps["images"]["interlace"].tolist() == [1, 0] * k
    for i in range(k):
        assert torch.equal(got[2 * i], batch[0][i]) and torch.equal(got[2 * i].cpu(), want[i]), names[i]
        assert torch.equal(got[2 * i + 1], plain_only[i]) and torch.equal(got[2 * i + 1].cpu(), torch.from_numpy(pz["bgr_" + pnames[i]])), pnames[i]
    flagged = M.png.decode(pfiles, device=DEV, interlaced=True)        # the flag alone changes nothing for plain files
    assert all(torch.equal(a, b) for a, b in zip(flagged, plain_only))


def test_malformed_files_raise_with_the_predicted_bits(cases, malformed, tmp_path):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    assert len(bad_names) == N_MALFORMED
    for n, f, st in zip(bad_names, bad_files, bad_status):
        assert A.decode_stages(f)[3] == st and st != 0, n           # the rule book, on the CPU, first
        p = tmp_path / (n + ".png")
        p.write_bytes(f)
        with pytest.raises(M.MafError, match=r"file 1 \(.*%s\.png\): .*\(status 0x%x\)" % (n, st)) as e:
            M.png.decode([files[4], str(p), files[5]], device=DEV, interlaced=True)
        assert not isinstance(e.value, P.PngUnsupported) and P.status_text(st) in str(e.value), n


def test_status_words_and_the_good_files_of_the_same_call(cases, malformed):
    names, files, want, _ = cases
    bad_names, bad_files, bad_status = malformed
    good = [8, 20, len(files) - 1, 12, 3]
    mix = [files[good[0]], bad_files[0], files[good[1]], bad_files[1], files[good[2]], bad_files[2], files[good[3]], bad_files[3], files[good[4]]]
    taps = {}
    frames, status = M.png.decode(mix, device=DEV, check=False, taps=taps, interlaced=True)
    st = status.tolist()
    assert st[0::2] == [0] * 5 and st[1::2] == bad_status
    for k, i in enumerate(good):
        assert torch.equal(frames[2 * k].cpu(), want[i]), names[i]
    inflated = taps["inflated"].cpu().numpy()
    for k, f in enumerate(bad_files):                              # a zero-filled remainder, the pixels the rule book gives
        bgr, inf, _, _ = A.decode_stages(f)
        o = int(taps["images"][2 * k + 1]["inf_off"])
        assert np.array_equal(inflated[o:o + inf.size], inf), bad_names[k]
        assert torch.equal(frames[2 * k + 1].cpu(), torch.from_numpy(bgr)), bad_names[k]


def test_router_on_jpeg_plain_and_interlaced_files(cases, batch, golden):
    names, files, want, _ = cases
    jz, pz = golden("jpeg_cases"), golden("png_cases")
    jfiles = [jz["file_" + str(n)].tobytes() for n in jz["names"][:2]]
    plain = pz["file_rgb8_17x33"].tobytes()
    jframes = M.jpeg.decode(jfiles, device=DEV)
    mix = [files[8], jfiles[0], plain, files[0], jfiles[1]]
    expect = [batch[0][8], jframes[0], M.png.decode([plain], device=DEV)[0], batch[0][0], jframes[1]]
    got = M.frames.decode(mix, device=DEV, interlaced=True)
    assert len(got) == len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))
    got, status = M.frames.decode(mix, device=DEV, check=False, interlaced=True)
    assert status.tolist() == [0] * len(mix) and all(torch.equal(g, e) for g, e in zip(got, expect))
    with pytest.raises(P.PngUnsupported, match="Adam7"):
        M.frames.decode(mix, device=DEV)
