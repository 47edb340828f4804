"""CPU tests of the training augmentation (maf-yolo_amd/augment.py, csrc/augment.hip): the sampler against what the reference's own
__getitem__ drew and computed (tests/golden/augment_cases.npz, tools/make_golden_augment.py), the scope checks, the pixel restatement
(tests/augment_ref.py) on hand-derived cases, the C-ABI's argument checks (they run before anything touches the device) and the torch op's
fake kernel."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

import augment_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import augment as A
from maf_yolo_amd import lib

SETS = ("default", "nomosaic", "dymixup")


def _sampler(g, name):
    sizes = [tuple(int(v) for v in s) for s in g[name + "_sizes"]]
    counts = g[name + "_nlabels_in"]
    labels = np.split(g[name + "_labels_in"], np.cumsum(counts)[:-1])
    hyp = json.loads(str(g[name + "_hyp"]))
    return A.TrainAugment([l.astype(np.float32) for l in labels], sizes, hyp, 640), hyp


@pytest.mark.parametrize("name", SETS)
def test_sampler_equals_reference(golden, name):
    g = golden("augment_cases")
    aug, hyp = _sampler(g, name)
    ints, tiles, Ms, ss = g[name + "_int"], g[name + "_tiles"], g[name + "_M"], g[name + "_s"]
    want_labels = g[name + "_labels"]
    assert len(ints) >= 200
    seed = int(g[name + "_seed"])
    random.seed(seed)
    np.random.seed(seed)
    row = 0
    for k, it in enumerate(ints):
        index, mosaic, mixup, flipud, fliplr, hsv, nlab = (int(v) for v in it[:7])
        xca, yca, xcb, ycb, top, left, nw, nh, nwarp = (int(v) for v in it[7:])
        smp = aug.draw(index)
        assert smp.mosaic == bool(mosaic) and (len(smp.layers) == 2) == bool(mixup), k
        assert (smp.flipud, smp.fliplr, smp.gains is not None) == (bool(flipud), bool(fliplr), bool(hsv)), k
        for li, layer in enumerate(smp.layers):
            assert np.array_equal(layer.M, Ms[k, li]) and layer.s == ss[k, li], k
            if mosaic:
                assert layer.center == ((xca, yca), (xcb, ycb))[li], k
                got = [(t.frame[1],) + tuple(t.hw) for t in layer.tiles]
                assert got == [tuple(int(v) for v in t) for t in tiles[k, 4 * li:4 * li + 4]], k
        if not mosaic:
            t = smp.layers[0].tiles[0]
            assert t.frame[1] == index and aug.loaded_hw(index) == tuple(int(v) for v in tiles[k, 0, 1:]), k
            assert (t.x0, t.y0, t.hw) == (left, top, (nh, nw)), k
            assert nwarp == int((smp.layers[0].M != np.eye(3)).any())
        if mixup:
            assert smp.mix_r == g[name + "_r"][k]
        if hsv:
            assert np.array_equal(smp.gains, g[name + "_gain"][k]) and np.array_equal(smp.lut, g[name + "_lut"][k]), k
        got = np.zeros((len(smp.labels), 6), np.float32)
        got[:, 1:] = smp.labels
        assert got.shape[0] == nlab
        assert np.array_equal(got.astype(np.float64), want_labels[row:row + nlab].astype(np.float64)), k
        row += nlab
    assert row == len(want_labels)


def test_fixture_covers_the_branches(golden):
    g = golden("augment_cases")
    d, n, m = g["default_int"], g["nomosaic_int"], g["dymixup_int"]
    assert d[:, 1].all() and not n[:, 1].any() and m[:, 2].sum() >= 50 and m[:, 3].sum() >= 20 and d[:, 4].sum() >= 50
    loaded = g["nomosaic_tiles"][:, 0, 1:]
    assert ((n[:, 13] != loaded[:, 0]) | (n[:, 12] != loaded[:, 1])).any(), "no non-mosaic draw took letterbox's second resize"


def test_polygon_labels_and_mixup_above_one_raise():
    hyp = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
               mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)
    lab = [np.zeros((1, 5), np.float32)]
    with pytest.raises(M.MafError, match="polygon"):
        A.TrainAugment(lab, [(10, 10)], hyp, segments=[[np.zeros((4, 2))]])
    with pytest.raises(M.MafError, match="polygon"):
        A.TrainAugment([np.zeros((1, 9), np.float32)], [(10, 10)], hyp)
    with pytest.raises(M.MafError, match="mixup > 1"):
        A.TrainAugment(lab, [(10, 10)], dict(hyp, mixup=1.5))
    A.TrainAugment(lab, [(10, 10)], hyp, segments=[[]])               # empty segments: box labels


def test_invert_affine_matches_numpy():
    rs = np.random.RandomState(1)
    for _ in range(20):
        Mx = np.eye(3)
        Mx[:2] = rs.uniform(-2, 2, (2, 3))
        inv = np.array(A.invert_affine(Mx)).reshape(2, 3)
        want = np.linalg.inv(Mx)[:2]
        assert np.allclose(inv, want, rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------- the pixel restatement

def test_integer_translation_is_a_shifted_copy():
    rs = np.random.RandomState(0)
    src = rs.randint(0, 256, (50, 70, 3)).astype(np.uint8)
    tiles = [R.RefTile(src, 5, 7, 5 + 70, 7 + 50, -5, -7)]
    Mx = np.array([[1.0, 0, -3], [0, 1.0, 11], [0, 0, 1]])
    got = R.warp_canvas(tiles, A.invert_affine(Mx), 64)
    want = np.full((64, 64, 3), 114, np.uint8)
    canvas = np.full((200, 200, 3), 114, np.uint8)
    canvas[7:57, 5:75] = src
    for y in range(64):
        for x in range(64):
            cy, cx = y - 11, x + 3
            want[y, x] = canvas[cy, cx] if 0 <= cy < 200 and 0 <= cx < 200 else 114
    assert np.array_equal(got, want)


def test_grey_survives_hsv_with_unit_gains():
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v, v, v], -1)[None]
    lut = A.hsv_luts(np.ones(3))
    assert np.array_equal(R.hsv_augment(img, lut), img)
    col = np.random.RandomState(3).randint(0, 256, (1, 4000, 3)).astype(np.uint8)
    h, s, vv = R.bgr2hsv(col)
    assert h.max() < 180 and np.array_equal(vv, col.max(-1))


def test_flips_commute_with_the_index_map():
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (32, 32, 3)).astype(np.uint8)
    for ud in (False, True):
        for lr in (False, True):
            want = img[::-1] if ud else img
            want = want[:, ::-1] if lr else want
            assert np.array_equal(R.flip(img, ud, lr), want)
            assert np.array_equal(R.flip(R.flip(img, ud, lr), ud, lr), img)


def test_bilinear_table_sums_to_32768():
    t = R.bilinear_table()
    assert t.shape == (32, 32, 4) and (t.sum(-1) == 32768).all()


def test_mixup_blend_truncates_like_astype():
    a = np.array([[[200, 3, 255]]], np.uint8)
    b = np.array([[[100, 4, 255]]], np.uint8)
    r = 0.4999999
    assert np.array_equal(R.blend(a, b, r), (a * r + b * (1 - r)).astype(np.uint8))


# ---------------------------------------------------------------- boundary (no device touched)

def test_library_declares_the_augment_symbols():
    assert {"maf_augment_resize", "maf_mosaic_affine"} <= set(lib.EXPORTS)
    L = lib.load()
    assert L.maf_augment_sample_size() == C.sizeof(lib.MafAugmentSample)


def test_c_abi_rejects_bad_arguments_before_the_device():
    L = lib.load()
    s = lib.MafAugmentSample()
    with pytest.raises(M.MafError, match="null"):
        lib.check(L.maf_mosaic_affine(None, None, 1, 640, None, None))
    s.ntiles[0] = 0
    out = C.c_void_p(64)                                                   # never dereferenced: validation fails first
    with pytest.raises(M.MafError, match="tiles"):
        lib.check(L.maf_mosaic_affine(C.byref(s), C.c_void_p(64), 1, 640, out, None))
    s.ntiles[0] = 1
    t = s.tile[0][0]
    t.ptr, t.pitch, t.w, t.h = 64, 30, 10, 10
    t.x0, t.y0, t.x1, t.y1, t.dx, t.dy = 0, 0, 11, 10, 0, 0                # one column past the frame
    with pytest.raises(M.MafError, match="outside"):
        lib.check(L.maf_mosaic_affine(C.byref(s), C.c_void_p(64), 1, 640, out, None))
    t.x1 = 10
    with pytest.raises(M.MafError, match="multiple of 32"):
        lib.check(L.maf_mosaic_affine(C.byref(s), C.c_void_p(64), 1, 100, out, None))
    f = lib.MafAugmentFrame(src=64, src_pitch=2, h=4, w=4, dst=64, new_h=2, new_w=2)
    with pytest.raises(M.MafError, match="pitch"):
        lib.check(L.maf_augment_resize(C.byref(f), C.c_void_p(64), 1, None))


def test_train_batch_has_no_cpu_fallback():
    hyp = dict(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
               mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)
    aug = A.TrainAugment([np.zeros((0, 5), np.float32)], [(8, 8)], hyp, 64)
    with pytest.raises(M.MafError, match="CUDA"):
        M.train_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], [0], aug)


def test_torch_op_fake_kernel():
    from maf_yolo_amd import torch_ops
    ops = torch_ops.load()
    assert hasattr(ops, "mosaic_affine")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        tab = torch.empty(3, C.sizeof(lib.MafAugmentSample), dtype=torch.uint8)
        out = ops.mosaic_affine(tab, tab.to("cuda"), 640)
        assert tuple(out.shape) == (3, 3, 640, 640) and out.dtype == torch.uint8
