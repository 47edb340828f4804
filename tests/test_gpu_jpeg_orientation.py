"""-m gpu: jpeg.decode(..., apply_orientation=True) on the device (the final store of jpeg_color_kernel, csrc/jpeg_decode.hip) against the
frames of tests/golden/jpeg_orientation_cases.npz (PIL.ImageOps.exif_transpose of Pillow's decode, stored BGR).  Bit-exact: torch.equal.

* orientations 2 to 8 on 13x22 at 4:2:0, 17x9 at 4:4:4, 9x14 at 4:2:2 and a 5x11 gray file (non-square, no side an MCU multiple), on a
  one-pixel-wide and a one-pixel-high frame, and on one progressive file each (progressive=True), in one call and alone;
* orientations 1, 6 and 3 side by side in one call; check=False returns the same frames and zero status words;
* files without a tag decode as without the flag; ignore_orientation still gives the stored grid, of which the flagged frame is the permutation;
* frames.decode(..., apply_orientation=True) equals the decoder's own output.
"""
import pytest
import torch

import jpeg_orientation_ref as O
import maf_yolo_amd as M
from maf_yolo_amd import jpeg as J

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_CASES, N_PROGRESSIVE = 51, 8        # the counts tools/make_golden_jpeg_orientation.py wrote: no case can drop out silently


@pytest.fixture(scope="module")
def cases(golden):
    z = golden("jpeg_orientation_cases")
    names = [str(n) for n in z["names"]]
    return names, [z["file_" + n].tobytes() for n in names], [torch.from_numpy(z["bgr_" + n]) for n in names], z["meta"].tolist()


@pytest.fixture(scope="module")
def batch(cases):
    """All cases, the progressive ones among them, decoded in ONE call (shared by the tests below; never modified)."""
    taps = {}
    return M.jpeg.decode(cases[1], device=DEV, progressive=True, apply_orientation=True, taps=taps), taps


def _check(names, frames, want, meta):
    done = 0
    for n, got, w, (h, wd, o, _) in zip(names, frames, want, meta):
        assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous(), n
        assert tuple(got.shape) == tuple(w.shape) == ((wd, h, 3) if o >= 5 else (h, wd, 3)), n
        assert torch.equal(got.cpu(), w), n
        done += 1
    return done


def test_every_case_in_one_call_is_bit_exact(cases, batch):
    names, files, want, meta = cases
    assert len(names) == len(batch[0]) == N_CASES and sum(m[3] for m in meta) == N_PROGRESSIVE
    assert sorted({m[2] for m in meta if m[3]}) == list(range(1, 9))      # one progressive file per orientation
    assert _check(names, batch[0], want, meta) == N_CASES
    taps = batch[1]
    assert int(taps["status"].abs().sum()) == 0
    # the views' table has the frames' sides; the allocation is 3 * w * h bytes per file either way
    assert [(int(im["h"]), int(im["w"])) for im in taps["images"]] == [tuple(w.shape[:2]) for w in want]
    assert int(taps["header"]["out_bytes"]) == sum(J._align(3 * m[0] * m[1]) for m in meta)


def test_baseline_cases_without_the_progressive_flag_and_each_alone(cases, batch):
    names, files, want, meta = cases
    pick = [i for i, m in enumerate(meta) if not m[3]]
    assert len(pick) == N_CASES - N_PROGRESSIVE
    frames = M.jpeg.decode([files[i] for i in pick], device=DEV, apply_orientation=True)
    assert _check([names[i] for i in pick], frames, [want[i] for i in pick], [meta[i] for i in pick]) == len(pick)
    done = 0
    for i, (n, f, b) in enumerate(zip(names, files, batch[0])):
        got = M.jpeg.decode([f], device=DEV, progressive=bool(meta[i][3]), apply_orientation=True)[0]
        assert torch.equal(got, b), n
        done += 1
    assert done == N_CASES


def test_orientations_1_6_and_3_side_by_side_and_check_false(cases, batch):
    names, files, want, meta = cases
    pick = [names.index(n) for n in ("o1_s2_13x22", "o6_s2_13x22", "o3_s2_13x22", "o6_prog_s2_13x22", "o1_prog_s2_13x22", "o3_gray_5x11")]
    frames, status = M.jpeg.decode([files[i] for i in pick], device=DEV, progressive=True, apply_orientation=True, check=False)
    assert status.dtype == torch.int32 and status.tolist() == [0] * len(pick)
    assert [tuple(f.shape) for f in frames] == [(13, 22, 3), (22, 13, 3), (13, 22, 3), (22, 13, 3), (13, 22, 3), (5, 11, 3)]
    for i, f in zip(pick, frames):
        assert torch.equal(f, batch[0][i]) and torch.equal(f.cpu(), want[i]), names[i]
    s = torch.cuda.Stream(DEV)
    frames, status = M.jpeg.decode(files, device=DEV, stream=s, progressive=True, apply_orientation=True, check=False)
    s.synchronize()
    assert status.tolist() == [0] * N_CASES and all(torch.equal(a, b) for a, b in zip(frames, batch[0]))


def test_the_flag_permutes_the_stored_grid_and_leaves_untagged_files_alone(cases, batch, golden):
    names, files, want, meta = cases
    stored = M.jpeg.decode(files, device=DEV, progressive=True, ignore_orientation=True)
    for n, s, b, (h, w, o, _) in zip(names, stored, batch[0], meta):
        assert tuple(s.shape) == (h, w, 3), n
        assert torch.equal(torch.from_numpy(O.orient(s.cpu().numpy(), o)), b.cpu()), n
    jz = golden("jpeg_cases")
    plain = [jz["file_" + str(n)].tobytes() for n in jz["names"][:6]]
    a, b = M.jpeg.decode(plain, device=DEV), M.jpeg.decode(plain, device=DEV, apply_orientation=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(J.JpegUnsupported, match="orientation 6"):
        M.jpeg.decode([files[names.index("o6_s2_13x22")]], device=DEV)


def test_router_hands_the_flag_on(cases, batch, golden):
    names, files, want, meta = cases
    png_file = golden("png_cases")["file_rgb8_3x5"].tobytes()
    pick = [names.index(n) for n in ("o6_s0_17x9", "o8_s2_7x1", "o5_s0_1x7")]
    mix = [files[pick[0]], png_file, files[pick[1]], files[pick[2]]]
    got = M.frames.decode(mix, device=DEV, apply_orientation=True)
    assert [tuple(g.shape) for g in got] == [(9, 17, 3), (5, 3, 3), (1, 7, 3), (7, 1, 3)]
    for g, i in zip([got[0], got[2], got[3]], pick):
        assert torch.equal(g, batch[0][i]), names[i]
    got, status = M.frames.decode(mix, device=DEV, apply_orientation=True, check=False)
    assert status.tolist() == [0] * 4 and torch.equal(got[0], batch[0][pick[0]])
