"""CPU tests of the INTER_AREA evaluation path (maf-yolo_amd/letterbox.py resize_area / eval_batch(area=True), csrc/resize_area.hip): the host
geometry with the new parameters against what the reference's own loader computed (tests/golden/area_cases.npz, tools/make_golden_area.py),
the decimation-table builder, the pixel restatement (tests/area_ref.py) against the float64 exact box average, and the argument checks of
the C-ABI (no GPU needed: they run before anything touches the device)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import area_ref as A
import letterbox_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import lib

LB = importlib.import_module("maf_yolo_amd.letterbox")


# ---------------------------------------------------------------- geometry vs the reference

def test_eval_geometry_with_area_equals_reference(golden):
    z = golden("area_cases")
    rows, seen, loads = z["rows"], 0, set()
    for ci, img_size, load_size, rect, pad, ret_int, nframes in z["cases"]:
        mine = rows[rows[:, 0] == ci]
        assert len(mine) == nframes
        hw0 = [(int(r[1]), int(r[2])) for r in mine]
        bs = LB.rect_batch_shape(hw0, int(img_size), 32, pad) if rect else [int(img_size)] * 2
        for r in mine:
            h0, w0, h, w, nload, interp, H, W, nuw, nuh, nlb, top, left = (int(v) for v in r[1:14])
            assert bs == [H, W]
            assert LB.load_image_size(h0, w0, int(img_size), int(load_size), area=True)[1] == (h, w)
            g = LB.eval_geometry(h0, w0, bs, int(img_size), load_size=int(load_size), return_int=bool(ret_int), area=True)
            assert g["load"] == {3: "area", 1: "linear", -1: None}[interp] and (nload == 1) == (g["load"] is not None)
            assert g["load_hw"] == (h, w) and g["new_unpad"] == (nuw, nuh) and g["shape"] == (H, W) and (g["top"], g["left"]) == (top, left)
            assert (nlb == 1) == (g["new_unpad"] != (w, h))
            assert g["shapes"] == ((int(r[14]), int(r[15])), ((r[16], r[17]), (r[18], r[19])))
            if ret_int:
                assert all(isinstance(p, int) for p in g["shapes"][1][1])
            loads.add((g["load"], nlb))
            seen += 1
    assert seen == len(rows) > 50 and {("area", 0), ("area", 1), ("linear", 0), (None, 0)} <= loads
    # the load size lands one below test_load_size by floating point on these two
    assert LB.load_image_size(1041, 800, 640, 638, area=True)[1] == (637, 490) and LB.load_image_size(700, 1069, 640, 630, area=True)[1] == (412, 629)


def test_defaults_are_unchanged():
    with pytest.raises(M.MafError, match="INTER_AREA"):
        LB.eval_geometry(1080, 1920, [384, 640], 640)
    with pytest.raises(M.MafError, match="resize twice"):
        LB.eval_geometry(480, 640, [320, 320], 640)
    with pytest.raises(M.MafError, match="INTER_AREA"):
        LB.load_image_size(480, 640, 640, load_size=638)
    with pytest.raises(M.MafError, match="resize twice"):         # area=True lifts it for frames that took the area path only
        LB.eval_geometry(100, 100, [128, 128], 128, load_size=160, area=True)
    assert LB.load_image_size(333, 500, 640) == (1.28, (426, 640)) and LB.load_image_size(480, 640) == (1.0, (480, 640))
    g = LB.eval_geometry(480, 640, [480, 640])
    assert g["load"] is None and g["shapes"] == ((480, 640), ((1.0, 1.0), (0.0, 0.0)))


def test_zero_side_raises():
    with pytest.raises(M.MafError, match="empty size"):
        LB.load_image_size(1, 640, 640, 638, area=True)


# ---------------------------------------------------------------- the decimation table

@pytest.mark.parametrize("n_src,n_dst", [(64, 63), (48, 47), (7, 3), (5, 2), (100, 7), (37, 3), (640, 638), (480, 478), (1001, 1000), (9, 3), (64, 64),
                                         (1920, 638), (3, 1), (2, 1), (199, 1)])
def test_table_builder(n_src, n_dst):
    start, si, alpha = LB.area_table(n_src, n_dst)
    ref = A.area_tab(n_src, n_dst)
    assert start.dtype == np.int32 and si.dtype == np.int32 and alpha.dtype == np.float32 and start[0] == 0 and len(start) == n_dst + 1
    scale = 1.0 / (n_dst / n_src)
    for d in range(n_dst):
        e_si, e_al = si[start[d]:start[d + 1]], alpha[start[d]:start[d + 1]]
        assert [(int(s), a) for s, a in zip(e_si, e_al)] == [(s, a) for s, a in ref[d]]          # the restatement's loop, entry for entry
        assert len(e_si) >= 1 and np.array_equal(e_si, np.arange(e_si[0], e_si[0] + len(e_si)))    # contiguous and ordered
        assert 0 <= e_si[0] and e_si[-1] < n_src and (e_al > 0).all()
        # the alphas sum to 1; a partial cell of at most 1e-3 source pixels that the cut dropped is the one thing that may be missing
        lo, hi = d * scale, min(d * scale + scale, n_src)
        kept = min(hi, e_si[-1] + 1) - max(lo, e_si[0])
        cell = min(scale, n_src - lo)
        assert abs(float(e_al.astype(np.float64).sum()) - kept / cell) < 1e-6
        assert (hi - lo) - kept <= 2e-3 + 1e-9
        if (n_src, n_dst) != (1001, 1000):
            assert abs(float(e_al.astype(np.float64).sum()) - 1.0) < 1e-6


def test_table_cut_at_1e_3():
    """1001 -> 1000: scale = 1.001 in double.  At dx = 999 fsx1 = 999.9989999999999 and sx1 - fsx1 = 0.00100000000009..., above the cut:
    the head entry (999, 0.000999001) is kept.  At dx = 0 fsx2 - sx2 = 0.00099999999999989, below it: the tail entry is dropped and the
    index owns the single entry (0, 1 / 1.001).  Both are what the double arithmetic gives, computed here and not assumed."""
    scale = 1.0 / (1000 / 1001)
    f1 = 999 * scale
    assert math.ceil(f1) - f1 > 1e-3 and abs((math.ceil(f1) - f1) - 1e-3) < 1e-9
    assert (0 * scale + scale) - 1 < 1e-3 and abs(scale - 1 - 1e-3) < 1e-9
    start, si, alpha = LB.area_table(1001, 1000)
    assert list(si[start[999]:start[1000]]) == [999, 1000]
    assert alpha[start[999]] == np.float32((1000 - f1) / scale) and alpha[start[999] + 1] == np.float32(min(min(f1 + scale - 1000, 1.0), scale) / scale)
    assert list(si[start[0]:start[1]]) == [0] and alpha[0] == np.float32(1.0 / scale)
    assert list(si[start[500]:start[501]]) == [500, 501]


def test_area_plan_uses_opencvs_test():
    assert LB.area_plan(4, 4, 2, 2) == (lib.AREA_FAST2, 2, 2)
    assert LB.area_plan(1080, 1920, 360, 640) == (lib.AREA_FASTN, 3, 3)
    assert LB.area_plan(8, 12, 2, 3) == (lib.AREA_FASTN, 4, 4) and LB.area_plan(8, 12, 4, 3) == (lib.AREA_FASTN, 4, 2)
    assert LB.area_plan(5, 5, 5, 5) == (lib.AREA_FASTN, 1, 1)
    assert LB.area_plan(48, 64, 48, 63)[0] == lib.AREA_GENERAL and LB.area_plan(480, 640, 478, 638)[0] == lib.AREA_GENERAL
    for h, w, nh, nw in [(9, 6, 3, 2), (100, 37, 7, 3), (147, 49, 3, 7), (1000, 3000, 10, 1000)]:      # 1.0 / (nw / w) in double, as OpenCV writes it
        sx, sy, ix, iy, fast = A.scales(h, w, nh, nw)
        assert (LB.area_plan(h, w, nh, nw)[0] != lib.AREA_GENERAL) == fast


# ---------------------------------------------------------------- the restatement

def _exact(src, nw, nh):
    """The box average in float64: every source pixel weighted by its overlap with the destination cell."""
    def weights(n_src, n_dst):
        m, s = np.zeros((n_dst, n_src)), n_src / n_dst
        for d in range(n_dst):
            a, b = d * s, (d + 1) * s
            for i in range(int(math.floor(a)), min(int(math.ceil(b)), n_src)):
                m[d, i] = max(0.0, min(b, i + 1) - max(a, i))
        return m / s
    rows = np.einsum("yh,hwc->ywc", weights(src.shape[0], nh), src.astype(np.float64))
    return np.einsum("ywc,xw->yxc", rows, weights(src.shape[1], nw))


def test_restatement_constant_frames_stay_constant():
    for v in (0, 255):
        f = np.full((48, 64, 3), v, np.uint8)
        for nh, nw in [(47, 63), (24, 32), (16, 16), (48, 63), (7, 3), (48, 64)]:
            assert (A.resize_area(f, nw, nh) == v).all(), (v, nh, nw)
            assert (A.resize_area_general(f, nw, nh) == v).all(), (v, nh, nw)


def test_restatement_copy_and_2x():
    f = R.synth_frame(5, 7, 1)
    assert np.array_equal(A.resize_area(f, 7, 5), f)
    f = R.synth_frame(18, 14, 2)
    assert np.array_equal(A.resize_area(f, 7, 9), R.resize_linear(f, 7, 9))
    g = np.arange(16, dtype=np.uint8).reshape(4, 4, 1) * 9
    assert np.array_equal(A.resize_area(g, 2, 2)[..., 0], [[(0 + 9 + 36 + 45 + 2) >> 2, (18 + 27 + 54 + 63 + 2) >> 2],
                                                           [(72 + 81 + 108 + 117 + 2) >> 2, (90 + 99 + 126 + 135 + 2) >> 2]])


def test_restatement_integer_factor_by_hand():
    f = np.array([[1, 2, 3, 250, 251, 253], [4, 5, 6, 255, 255, 255], [7, 8, 10, 0, 0, 1]], np.uint8)[..., None]
    out = A.resize_area(f, 2, 1)[..., 0]                          # 3 x 3 blocks: sums 46 and 1520, times float32(1 / 9)
    inv = np.float32(1.0) / np.float32(9)
    assert out.tolist() == [[int(np.rint(np.float32(46) * inv)), int(np.rint(np.float32(1520) * inv))]] == [[5, 169]]


@pytest.mark.parametrize("hw,nhw", [((48, 64), (47, 63)), ((7, 5), (3, 2)), ((100, 37), (7, 3)), ((9, 6), (3, 2)), ((480, 640), (478, 638))])
def test_restatement_within_one_of_exact_box_average(hw, nhw):
    f = R.synth_frame(hw[0], hw[1], 11)
    got = A.resize_area(f, nhw[1], nhw[0]).astype(np.int64)
    assert got.shape == (nhw[0], nhw[1], 3)
    assert np.abs(got - np.rint(_exact(f, nhw[1], nhw[0])).astype(np.int64)).max() <= 1


@pytest.mark.parametrize("hw,nhw", [((9, 6), (3, 2)), ((8, 12), (2, 3)), ((4, 4), (2, 2)), ((5, 5), (5, 5)), ((720, 1280), (360, 640))])
def test_restatement_general_path_on_integer_factors_within_one(hw, nhw):
    f = R.synth_frame(hw[0], hw[1], 12)
    assert A.scales(hw[0], hw[1], nhw[0], nhw[1])[4]
    d = A.resize_area_general(f, nhw[1], nhw[0]).astype(np.int64) - A.resize_area(f, nhw[1], nhw[0])
    assert np.abs(d).max() <= 1


def test_restatement_1080p_is_quick():
    import time
    f = R.synth_frame(1080, 1920, 13)
    t = time.perf_counter()
    out = A.resize_area(f, 640, 360)
    assert time.perf_counter() - t < 1.0 and out.shape == (360, 640, 3)


def test_load_letterbox_pixels_composes():
    f = R.synth_frame(40, 30, 14)
    out = A.load_letterbox_pixels(f, (12, 16), (6, 8), 4, 5, 32, 32)          # area to 16 x 12, then the exact-2x linear rule to 8 x 6
    small = R.resize_linear(A.resize_area(f, 12, 16), 6, 8)
    assert out.shape == (3, 32, 32) and np.array_equal(out[::-1, 4:12, 5:11].transpose(1, 2, 0), small) and (out[:, :4] == 114).all()


# ---------------------------------------------------------------- error paths (no device touched)

def test_cpu_frames_raise():
    with pytest.raises(M.MafError, match="no CPU fallback"):
        M.resize_area([torch.zeros(4, 4, 3, dtype=torch.uint8)], [(2, 2)])
    with pytest.raises(M.MafError, match="no CPU fallback"):
        M.eval_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], 4, area=True)
    assert M.resize_area is LB.resize_area


def _frame(**kw):
    d = dict(src=0x1000, src_pitch=300, h=10, w=100, dst=0x9000, new_h=10, new_w=100, path=lib.AREA_FASTN, iscale_x=1, iscale_y=1, inv_area=1.0)
    d.update(kw)
    t = np.zeros(1, LB.AREA_FRAME_DT)
    for k, v in d.items():
        t[0][k] = v
    return t


@pytest.mark.parametrize("kw,n,msg", [
    (dict(src=0), 1, "null frame pointer"),
    (dict(dst=0), 1, "null frame pointer"),
    (dict(new_w=101), 1, "exceed the source"),
    (dict(new_h=11), 1, "exceed the source"),
    (dict(src_pitch=299), 1, "pitch"),
    (dict(new_w=0), 1, "positive"),
    (dict(), 0, "n must be positive"),
    (dict(), -3, "n must be positive"),
    (dict(new_w=50), 1, "exact integer factors"),
    (dict(path=lib.AREA_FAST2), 1, "both factors 2"),
    (dict(path=7), 1, "unknown path"),
    (dict(path=lib.AREA_GENERAL, new_w=99), 1, "needs the decimation tables"),
])
def test_c_abi_resize_area_rejects_bad_arguments(kw, n, msg):
    L = lib.load()
    t = _frame(**kw)
    rc = L.maf_resize_area(t.ctypes.data, C.c_void_p(0x4000), n, None, None, 0, None)
    assert rc != 0 and msg in L.maf_last_error().decode()


def test_c_abi_resize_area_rejects_null_tables_and_bad_table_words():
    L = lib.load()
    t = _frame()
    assert L.maf_resize_area(None, C.c_void_p(0x4000), 1, None, None, 0, None) != 0 and "null pointer" in L.maf_last_error().decode()
    assert L.maf_resize_area(t.ctypes.data, None, 1, None, None, 0, None) != 0 and "null pointer" in L.maf_last_error().decode()
    # a general-path frame 4 x 3 -> 2 x 2 whose tables are checked word by word on the host copy
    xs, xsi, xal = LB.area_table(3, 2)
    ys, ysi, yal = LB.area_table(4, 2)

    def words(xsi=xsi, xs=xs):
        xp, yp = np.empty(2 * xsi.size, np.int32), np.empty(2 * ysi.size, np.int32)
        xp[0::2], xp[1::2], yp[0::2], yp[1::2] = xsi, xal.view(np.int32), ysi, yal.view(np.int32)
        return np.concatenate([xs, [0], xp, ys, [0], yp]).astype(np.int32), (0, 4, 4 + xp.size, 4 + xp.size + 4)

    for bad, kw in [("index", dict(xsi=np.array([0, 1, 1, 3], np.int32))), ("start", dict(xs=np.array([0, 2, 2], np.int32))),
                    ("offset", None), ("odd", None)]:
        w, (a, b, c, d) = words(**(kw or {}))
        if bad == "offset":
            d = len(w) - 2
        if bad == "odd":
            b += 1
        t = _frame(h=4, w=3, new_h=2, new_w=2, src_pitch=9, path=lib.AREA_GENERAL, x_start=a, x_pairs=b, y_start=c, y_pairs=d)
        rc = L.maf_resize_area(t.ctypes.data, C.c_void_p(0x4000), 1, w.ctypes.data, C.c_void_p(0x8000), len(w), None)
        assert rc != 0 and "decimation table" in L.maf_last_error().decode(), bad
    size = (C.c_int32 * 1)()
    assert L.maf_area_struct_sizes(size) == 0 and size[0] == LB.AREA_FRAME_DT.itemsize == 72
