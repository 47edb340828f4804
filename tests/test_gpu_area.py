"""-m gpu: OpenCV's INTER_AREA shrink on the device (csrc/resize_area.hip) and the evaluation loader that uses it
(maf-yolo_amd/letterbox.py resize_area, eval_batch(area=True)).

* resize_area equals the NumPy restatement (tests/area_ref.py) bit for bit on the 2 x 2 path, the integer-factor path, the decimation-table
  path, one axis an exact 1, one-pixel rows and columns, the 1e-3 cut of 1001 -> 1000, constant frames, cropped views with odd offsets and a
  mixed batch of 70 frames where every path shares one launch;
* eval_batch(area=True, ...) equals the composed restatement (area, then letterbox) and the `shapes` the reference's loader computed
  (tests/golden/area_cases.npz); decoded JPEG frames go straight in;
* nothing synchronises the host; one end-to-end run down to coco_rows(scale_exact=True) against the oracle.
"""
import importlib

import numpy as np
import pytest
import torch

import area_ref as A
import letterbox_ref as R
import maf_yolo_amd as M
from oracle import maf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LB = importlib.import_module("maf_yolo_amd.letterbox")


def _check(host, sizes):
    got = M.resize_area([torch.from_numpy(f).to(DEV) for f in host], sizes)
    assert len(got) == len(host)
    for f, (nh, nw), g in zip(host, sizes, got):
        assert g.dtype == torch.uint8 and tuple(g.shape) == (nh, nw, 3) and g.is_cuda
        assert np.array_equal(g.cpu().numpy(), A.resize_area(f, nw, nh)), (f.shape, nh, nw)
    return got


@pytest.mark.parametrize("hw,nhw", [((4, 4), (2, 2)), ((9, 6), (3, 2)), ((8, 12), (2, 3)), ((3, 3), (1, 1)), ((5, 5), (5, 5)), ((7, 5), (3, 2)),
                                    ((48, 64), (47, 63)), ((48, 64), (48, 63)), ((1, 64), (1, 63)), ((64, 1), (63, 1)), ((3, 1001), (3, 1000)),
                                    ((100, 37), (7, 3)), ((720, 1280), (360, 640)), ((480, 640), (478, 638)), ((1080, 1920), (360, 640))])
def test_resize_area_equals_restatement(hw, nhw):
    got = _check([R.synth_frame(hw[0], hw[1], 5)], [nhw])
    assert got[0].is_contiguous()


def test_constant_frames_stay_constant():
    host, sizes = [], []
    for v in (0, 255):
        for nhw in [(47, 63), (24, 32), (16, 16), (48, 63), (7, 3), (48, 64)]:
            host.append(np.full((48, 64, 3), v, np.uint8))
            sizes.append(nhw)
    for g, f in zip(_check(host, sizes), host):
        assert (g == int(f[0, 0, 0])).all()


def test_cropped_views_with_odd_offsets_and_pitch():
    big_host = R.synth_frame(300, 400, 6)
    big = torch.from_numpy(big_host).to(DEV)
    cuts = [(slice(3, 200), slice(5, 300)), (slice(1, 49), slice(1, 65)), (slice(7, 107), slice(9, 46)), (slice(0, 300), slice(1, 400)),
            (slice(11, 131), slice(3, 243)), (slice(5, 6), slice(7, 8))]
    sizes = [(101, 77), (24, 32), (7, 3), (299, 398), (40, 80), (1, 1)]                    # general, 2 x 2, general, general, 3 x 3, copy
    views = [big[a, b] for a, b in cuts]
    assert all(v.stride(0) == 1200 > 3 * v.shape[1] for v in views)
    got = M.resize_area(views, sizes)
    for (a, b), (nh, nw), g in zip(cuts, sizes, got):
        assert np.array_equal(g.cpu().numpy(), A.resize_area(big_host[a, b], nw, nh))
    assert np.array_equal(big.cpu().numpy(), big_host)                                      # the sources are untouched
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1                          # views of one allocation


def test_mixed_batch_of_70_every_path_in_one_launch():
    rs = np.random.RandomState(70)
    host, sizes, paths = [], [], set()
    for i in range(70):
        h, w = int(rs.randint(1, 200)), int(rs.randint(1, 200))
        kind = i % 4
        if kind == 0:                                                                       # exact integer factors, 2 x 2 among them
            k = int(rs.randint(1, 5))
            h, w = max(h // k, 1) * k, max(w // k, 1) * k
            nh, nw = h // k, w // k
        else:
            nh, nw = int(rs.randint(1, h + 1)), int(rs.randint(1, w + 1))
        host.append(R.synth_frame(h, w, 100 + i))
        sizes.append((nh, nw))
        paths.add(LB.area_plan(h, w, nh, nw)[0])
    assert paths == {0, 1, 2}
    _check(host, sizes)


def test_resize_area_rejects_growing_axes_and_zero_sizes():
    f = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    for size in [(9, 8), (8, 9), (0, 4), (4, 0)]:
        with pytest.raises(M.MafError):
            M.resize_area([f], [size])
    with pytest.raises(M.MafError):
        M.resize_area([f.float()], [(4, 4)])


# ---------------------------------------------------------------- eval_batch(area=True)

def _want_batch(host, img_size, **kw):
    """The composed restatement for eval_batch(frames, img_size, area=True, **kw) -> (uint8 [B, 3, H, W], geometries)."""
    hw0 = [f.shape[:2] for f in host]
    if kw.get("shape") is not None:
        bs = list(kw["shape"])
    elif not kw.get("rect", True):
        bs = [img_size, img_size]
    else:
        bs = LB.rect_batch_shape(hw0, img_size, 32, kw.get("pad", 0.5))
    out, geoms = [], []
    for f in host:
        g = LB.eval_geometry(f.shape[0], f.shape[1], bs, img_size, kw.get("load_size"), kw.get("return_int", False), True)
        if g["load"] == "area":
            px = A.load_letterbox_pixels(f, g["load_hw"][::-1], g["new_unpad"], g["top"], g["left"], bs[0], bs[1])
        else:
            px = R.letterbox_pixels(f, g["new_unpad"], g["top"], g["left"], bs[0], bs[1])
        out.append(px)
        geoms.append(g)
    return np.stack(out), geoms


def _fixture_shapes(golden, case, hw0):
    rows = golden("area_cases")["rows"]
    out = []
    for h0, w0 in hw0:
        r = rows[(rows[:, 0] == case) & (rows[:, 1] == h0) & (rows[:, 2] == w0)][0]
        pad = (r[18], r[19])
        out.append(((int(r[14]), int(r[15])), ((r[16], r[17]), pad)))
    return tuple(out)


def _eval_case(golden, case, sizes, img_size, seed, loads, **kw):
    host = [R.synth_frame(h, w, seed + i) for i, (h, w) in enumerate(sizes)]
    imgs, shapes = M.eval_batch([torch.from_numpy(f).to(DEV) for f in host], img_size, area=True, **kw)
    want, geoms = _want_batch(host, img_size, **kw)
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == want.shape
    assert np.array_equal(imgs.cpu().numpy(), want)
    assert shapes == tuple(g["shapes"] for g in geoms) == _fixture_shapes(golden, case, sizes)
    assert [g["load"] for g in geoms] == loads
    return geoms


def test_eval_batch_reproduce_settings(golden):
    _eval_case(golden, 2, [(48, 64), (64, 43), (64, 64)], 64, 20, ["area"] * 3, pad=0.0, rect=False, load_size=62, return_int=True)


def test_eval_batch_rect_mixed_larger_and_smaller(golden):
    _eval_case(golden, 4, [(200, 300), (96, 128), (150, 180), (64, 100), (1080, 1920), (128, 128)], 128, 30,
               ["area", None, "area", "linear", "area", None])


def test_eval_batch_letterbox_shrinks_again_after_the_area_step(golden):
    g = _eval_case(golden, 7, [(400, 300), (200, 320), (640, 640), (161, 97)], 128, 40, ["area"] * 4, pad=0.0, rect=False, load_size=160,
                   return_int=True)
    assert all(x["new_unpad"] != x["load_hw"][::-1] for x in g)


def test_eval_batch_without_area_still_raises():
    f = torch.zeros(200, 300, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(M.MafError, match="INTER_AREA"):
        M.eval_batch([f], 128)
    with pytest.raises(M.MafError, match="INTER_AREA"):
        M.eval_batch([f], 128, load_size=126, rect=False)


def test_decoded_jpegs_go_straight_in(golden):
    z = golden("jpeg_cases")
    names = ["grad_q75_75x100_s1", "noise_q30_opt_48x64_s0", "grad_q75_17x33_s2", "noise_q30_opt_75x100_s2"]
    frames = M.jpeg.decode([z["file_" + n].tobytes() for n in names], device=DEV)
    up = [torch.from_numpy(z["bgr_" + n]).to(DEV) for n in names]
    kw = dict(area=True, rect=False, pad=0.0, load_size=62, return_int=True)
    a, sa = M.eval_batch(frames, 64, **kw)
    b, sb = M.eval_batch(up, 64, **kw)
    assert torch.equal(a, b) and sa == sb
    want, _ = _want_batch([z["bgr_" + n] for n in names], 64, rect=False, pad=0.0, load_size=62, return_int=True)
    assert np.array_equal(a.cpu().numpy(), want)


# ---------------------------------------------------------------- no host sync, end to end

def test_no_host_sync():
    dev = [torch.from_numpy(R.synth_frame(h, w, 50 + i)).to(DEV) for i, (h, w) in enumerate([(48, 64), (64, 43), (90, 120), (30, 40)])]
    kw = dict(area=True, rect=False, pad=0.0, load_size=62, return_int=True)
    M.resize_area(dev[:3], [(47, 63), (32, 21), (30, 40)])          # warm: library loaded, pinned pool primed
    M.eval_batch(dev, 64, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        small = M.resize_area(dev[:3], [(47, 63), (32, 21), (30, 40)])
        imgs, _ = M.eval_batch(dev, 64, **kw)
        with pytest.raises(RuntimeError):                           # the check is live
            imgs.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert np.array_equal(small[0].cpu().numpy(), A.resize_area(dev[0].cpu().numpy(), 63, 47))


def test_reproduce_style_eval_batch_to_coco_rows():
    model = M.Model("n")
    model.load_state_dict(O.synth_state_dict("n", 0))
    model = model.to(DEV).eval()
    sizes = [(480, 640), (640, 427), (333, 500)]
    dev = [torch.from_numpy(R.synth_frame(h, w, 60 + i)).to(DEV) for i, (h, w) in enumerate(sizes)]
    imgs, shapes = M.eval_batch(dev, 320, pad=0.0, rect=False, area=True, load_size=318, return_int=True)
    assert tuple(imgs.shape) == (3, 3, 320, 320)
    with torch.no_grad():
        pred = model(imgs)[0]
    raw = M.nms_raw(pred, 0.03, 0.65, multi_label=True)
    ids = list(range(1, 81))
    res = M.convert_to_coco_format(raw, imgs, ["1.jpg", "2.jpg", "3.jpg"], shapes, ids, scale_exact=True)
    counts = raw[2].tolist()
    outs = [raw[0][b, :n].cpu().numpy() for b, n in enumerate(counts)]
    iid, cid, bb, sc = O.coco_rows(outs, shapes, [1, 2, 3], ids, scale_exact=True)
    assert len(res) == sum(counts) > 0 and [r["image_id"] for r in res] == iid.tolist() and [r["category_id"] for r in res] == cid.tolist()
    assert np.array_equal(np.asarray([r["bbox"] for r in res]).reshape(-1, 4), bb) and np.array_equal(np.asarray([r["score"] for r in res]), sc)
