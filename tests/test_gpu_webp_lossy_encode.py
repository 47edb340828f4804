"""-m gpu: lossy WebP (VP8) encoding on the device (csrc/vp8_encode.hip, maf-yolo_amd/webp_lossy_encode.py) against the files and taps the rule
book (tests/webp_lossy_encode_ref.py) wrote into tests/golden/webp_lossy_encode_cases.npz.  Byte-exact: ==, no tolerance.

* every fixture case (1x1 ... 130x70; padding on both axes, skips, 1 to 8 partitions, the largest tokens at base_q 0, the coarsest quantiser, the
  largest Y2 DC; filter_level default and 0), the cases that share their arguments in ONE call (a batch of mixed sizes), and each alone;
* the taps (the Y, U, V planes that went in, modes, levels, skip flags, the unfiltered reconstruction, partition sizes) equal the fixture's, so
  a byte mismatch points at its stage;
* webp_lossy.decode of the files on the device equals Pillow's decode of the same bytes;
* 40 rectangles of 5 to 40 pixels a side out of two frames with different row pitch equal the encodes of the cropped tensors;
* a second stream; frames.encode with webp_lossy=True keeps input order among other suffixes.
The status bit of a partition overflow is not provoked here: the bound's test is the host one.
"""
import io

import numpy as np
import pytest
import torch

import webp_lossy_encode_ref as R
from maf_yolo_amd import frames as F, jpeg_encode, png_encode, webp_lossy, webp_lossy_encode as E
from maf_yolo_amd.lib import MafError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _kw(args):
    base_q, level, lp = (int(v) for v in args)
    return dict(base_q=base_q, filter_level=None if level < 0 else level, log2_parts=lp)


@pytest.fixture(scope="module")
def cases(golden):
    """{arguments: [(name, frame on the device, the fixture's file)]}: one call takes one set of arguments."""
    z = golden("webp_lossy_encode_cases")
    groups = {}
    for name, args in zip((str(n) for n in z["names"]), z["args"].tolist()):
        groups.setdefault(tuple(args), []).append((name, torch.from_numpy(z["frame_" + name]).to(DEV), z["file_" + name].tobytes()))
    return groups, z


@pytest.fixture(scope="module")
def batches(cases):
    """Every set of arguments' cases encoded in ONE call, with the taps (shared by the tests below; never modified)."""
    out = {}
    for args, group in cases[0].items():
        taps = {}
        out[args] = (E.encode([g[1] for g in group], taps=taps, **_kw(args)), taps)
    return out


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def check_taps(z, name, taps, k):
    """The intermediate buffers of file `k` of a call against the fixture's taps, stage by stage."""
    job = taps["jobs"][k]
    mbw, mbh, o, mb0 = int(job["mbw"]), int(job["mbh"]), int(job["plane_off"]), int(job["mb0"])
    n = mbw * mbh
    shapes = ((16 * mbh, 16 * mbw), (8 * mbh, 8 * mbw), (8 * mbh, 8 * mbw))
    for buf, keys, what in ((taps["planes"], "yuv", "input plane"), (taps["recon"], ("ry", "ru", "rv"), "reconstruction")):
        at = o
        for key, (hh, ww) in zip(keys, shapes):
            got = buf[at:at + hh * ww].cpu().numpy().reshape(hh, ww)
            assert np.array_equal(got, z["%s_%s" % (key, name)]), "%s: %s %s" % (name, what, key)
            at += hh * ww
    info = taps["info"][mb0:mb0 + n].cpu().numpy().view(np.uint32)
    assert np.array_equal((info >> 25) & 3, z["ymodes_" + name]), "%s: luma modes" % name
    assert np.array_equal((info >> 27) & 3, z["uvmodes_" + name]), "%s: chroma modes" % name
    levels = taps["levels"][E.MB_LEVELS * mb0:E.MB_LEVELS * (mb0 + n)].cpu().numpy().reshape(n, 25, 16)
    assert np.array_equal(levels, z["levels_" + name]), "%s: levels" % name
    assert np.array_equal(info & 0x1ffffff, (np.abs(z["levels_" + name]).max(2) > 0).astype(np.uint32) @ (1 << np.arange(25, dtype=np.uint32))), "%s: non-zero flags" % name
    meta = taps["meta"].cpu().numpy().reshape(-1, E.META_WORDS)[k]
    parts = z["parts_" + name].tolist()
    zero = (info >> 29) & 1
    use_skip = (n - int(zero.sum())) * 255 // n < 250
    assert np.array_equal(zero if use_skip else 0 * zero, z["skips_" + name]), "%s: skip flags" % name
    assert meta[0] == int(zero.sum()) and meta[1] == 0 and meta[2:2 + len(parts)].tolist() == parts, "%s: skip count, status, partition sizes" % name


def test_every_case_in_one_call_per_arguments_is_byte_exact(cases, batches):
    groups, z = cases
    assert len(z["names"]) >= 15 and max(len(g) for g in groups.values()) >= 6
    assert any(len({tuple(g[1].shape) for g in group}) >= 3 for group in groups.values())          # one batch mixes three sizes (and more)
    for args, group in groups.items():
        enc, taps = batches[args]
        assert enc.buffer.is_cuda and enc.lengths.dtype == torch.int32 and len(enc) == len(group)
        files = enc.files()
        assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
        for k, ((name, _, want), got) in enumerate(zip(group, files)):
            check_taps(z, name, taps, k)
            assert got == want, name
        assert enc.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).tolist()


def test_each_case_alone_is_byte_exact(cases):
    for args, group in cases[0].items():
        for name, frame, want in group:
            assert E.encode([frame], **_kw(args)).files() == [want], name


def test_the_device_decoder_and_pillow_return_the_same_frame(cases, batches):
    for args, group in cases[0].items():
        files = batches[args][0].files()
        back = webp_lossy.decode(files, device=DEV)
        for (name, frame, _), data, got in zip(group, files, back):
            assert got.shape == frame.shape, name
            assert np.array_equal(got.cpu().numpy(), pillow_decode(data)), name


def test_rectangles_equal_the_encodes_of_the_crops():
    rng = np.random.default_rng(23)
    a = torch.from_numpy(rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)).to(DEV)
    wide = torch.from_numpy(rng.integers(0, 256, (50, 96, 3), dtype=np.uint8)).to(DEV)
    b = wide[:, 7:71]                                                                       # 64 wide, row pitch 288
    assert not b.is_contiguous() and a.stride(0) != b.stride(0)
    rects = []
    for k in range(40):
        f = k & 1
        fh, fw = (a, b)[f].shape[:2]
        w, h = (int(v) for v in rng.integers(5, 41, 2))
        x1, y1 = int(rng.integers(0, fw - w + 1)), int(rng.integers(0, fh - h + 1))
        rects.append((f, x1, y1, x1 + w, y1 + h))
    rects = np.array(rects)
    got = E.encode([a, b], base_q=30, rects=rects).files()
    crops = [(a, b)[f][y1:y2, x1:x2].contiguous() for f, x1, y1, x2, y2 in rects.tolist()]
    assert got == E.encode(crops, base_q=30).files()
    for k in (0, 1, 17):
        assert got[k] == R.encode(crops[k].cpu().numpy(), 30), k


def test_a_second_stream_and_a_batch_tensor(cases):
    args, group = max(cases[0].items(), key=lambda kv: len(kv[1]))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    assert E.encode([g[1] for g in group], stream=side, **_kw(args)).files() == [g[2] for g in group]
    frame = next(g for g in group if g[0] == "33x47")
    assert E.encode(torch.stack([frame[1], frame[1]]), **_kw(args)).files() == [frame[2]] * 2


def test_quality_maps_to_base_q(cases):
    frame = next(g for group in cases[0].values() for g in group if g[0] == "33x47")[1]
    assert E.encode([frame], quality=75).files() == E.encode([frame], base_q=26).files()
    assert E.encode([frame], quality=75, base_q=30).files() == E.encode([frame], base_q=30).files()          # base_q wins


def test_the_router_sends_webp_files_to_this_encoder(cases):
    groups, z = cases
    group = {g[0]: g for gr in groups.values() for g in gr}
    four = [group[n] for n in ("16x16", "33x47", "15x17", "64x48_flat")]
    fr = [g[1] for g in four]
    suffixes = [".jpg", ".webp", ".png", ".WEBP"]
    got = F.encode(fr, suffixes, webp_lossy=dict(base_q=30))
    assert got == [jpeg_encode.encode([fr[0]]).files()[0], four[1][2], png_encode.encode([fr[2]]).files()[0], four[3][2]]
    assert F.encode(fr, suffixes, webp_lossy=True)[1] == E.encode([fr[1]]).files()[0]
    with pytest.raises(MafError, match="no device encoder"):
        F.encode(fr, suffixes)
    with pytest.raises(MafError, match="both given"):
        F.encode(fr, suffixes, webp_lossy=True, webp_lossless=True)
