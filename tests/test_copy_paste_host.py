"""CPU tests of copy_paste and mask_refine on polygon labels (maf-yolo_amd/augment.py TrainAugment(polygons=True), csrc/polygon_mask.hip):
the sampler against what the reference's own __getitem__ drew, pasted and computed (tests/golden/copy_paste_cases.npz,
tools/make_golden_copy_paste.py); the fill rule of tests/copy_paste_ref.py against two independent judges (an exact integer even-odd
point-in-polygon test and Pillow's polygon fill) and against hand-written masks; the opt-in and the input validation; the C-ABI's argument
checks (they run before anything touches the device) and the torch ops' fake kernels."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

import copy_paste_ref as P
import maf_yolo_amd as M
from maf_yolo_amd import augment as A
from maf_yolo_amd import lib

SETS = ("n", "m", "stress")
HYP_N = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
             mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)


def _sampler(g, name):
    sizes = [tuple(int(v) for v in s) for s in g[name + "_sizes"]]
    counts = g[name + "_nlabels_in"]
    labels = np.split(g[name + "_labels_in"], np.cumsum(counts)[:-1])
    polys = np.split(g[name + "_seg_xy"], np.cumsum(g[name + "_seg_len"])[:-1])
    segments, k = [], 0
    for n in counts:
        segments.append(polys[k:k + int(n)])
        k += int(n)
    hyp = json.loads(str(g[name + "_hyp"]))
    return A.TrainAugment([l.astype(np.float32) for l in labels], sizes, hyp, 640, segments=segments, polygons=True)


@pytest.mark.parametrize("name", SETS)
def test_sampler_equals_reference(golden, name):
    g = golden("copy_paste_cases")
    aug = _sampler(g, name)
    ints, tiles, Ms, ss, ncont = g[name + "_int"], g[name + "_tiles"], g[name + "_M"], g[name + "_s"], g[name + "_ncontours"]
    contours = np.split(g[name + "_contour_xy"], np.cumsum(g[name + "_contour_len"])[:-1]) if len(g[name + "_contour_len"]) else []
    want_labels = g[name + "_labels"]
    assert len(ints) >= 100
    seed = int(g[name + "_seed"])
    random.seed(seed)
    np.random.seed(seed)
    row = cont = 0
    for k, it in enumerate(ints):
        index, mosaic, mixup, flipud, fliplr, hsv, nlab, xca, yca, xcb, ycb = (int(v) for v in it)
        smp = aug.draw(index)
        assert smp.mosaic == bool(mosaic) and (len(smp.layers) == 2) == bool(mixup), k
        assert (smp.flipud, smp.fliplr, smp.gains is not None) == (bool(flipud), bool(fliplr), bool(hsv)), k
        for li, layer in enumerate(smp.layers):
            assert np.array_equal(layer.M, Ms[k, li]) and layer.s == ss[k, li], k
            assert layer.center == ((xca, yca), (xcb, ycb))[li], k
            got = [(t.frame[1],) + tuple(t.hw) for t in layer.tiles]
            assert got == [tuple(int(v) for v in t) for t in tiles[k, 4 * li:4 * li + 4]], k
            assert len(layer.paste) == ncont[k, li], (k, li)
            for c in layer.paste:
                assert c.dtype == np.int32 and np.array_equal(c, contours[cont]), (k, li)
                cont += 1
        if not mixup:
            assert ncont[k, 1] == 0
        else:
            assert smp.mix_r == g[name + "_r"][k]
        if hsv:
            assert np.array_equal(smp.gains, g[name + "_gain"][k]) and np.array_equal(smp.lut, g[name + "_lut"][k]), k
        got = np.zeros((len(smp.labels), 6), np.float32)
        got[:, 1:] = smp.labels
        assert got.shape[0] == nlab, k
        assert np.array_equal(got.astype(np.float64), want_labels[row:row + nlab].astype(np.float64)), k
        row += nlab
    assert row == len(want_labels) and cont == len(contours)
    assert random.random() == float(g[name + "_after"])


def test_fixture_exercises_the_feature(golden):
    g = golden("copy_paste_cases")
    for name in SETS:
        nc, ex = g[name + "_ncontours"], g[name + "_extra"]
        assert (nc[:, 0] >= 1).sum() >= 10 and (nc[:, 1] >= 1).sum() >= 3, name
        assert (ex[:, 0] > 0).sum() >= 10, "segment2box never took its fallback in " + name
        assert (ex[:, 1] > 0).sum() >= 3, "box_candidates never dropped a pasted object in " + name
    hyps = {name: json.loads(str(g[name + "_hyp"])) for name in SETS}
    assert hyps["n"]["copy_paste"] == 0.05 and hyps["m"]["copy_paste"] == 0.2 and (hyps["m"]["mixup"], hyps["m"]["dy_mixup"]) == (0.1, 0.4)
    assert (hyps["stress"]["copy_paste"], hyps["stress"]["degrees"], hyps["stress"]["shear"]) == (1.0, 5.0, 2.0)
    assert all(h["mask_refine"] for h in hyps.values())


# ---------------------------------------------------------------- the fill rule against independent judges

CANVAS = 192


def _blob():
    rs = np.random.RandomState(3)
    t = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    r = 62 + 9 * np.sin(5 * t) + rs.uniform(-2, 2, 300)
    return np.stack([96 + r * np.cos(t), 96 + r * np.sin(t)], 1).round().astype(np.int32)


POLYGONS = {
    "convex": [(30, 20), (120, 12), (170, 70), (150, 160), (60, 175), (15, 100)],
    "concave": [(20, 20), (170, 25), (165, 170), (110, 165), (105, 80), (70, 85), (75, 160), (25, 170)],
    "bow_tie": [(20, 20), (160, 150), (160, 20), (20, 150)],
    "blob_300": _blob(),
    "left": [(-40, 30), (70, 50), (30, 150), (-30, 120)],
    "right": [(120, 30), (250, 60), (230, 170), (140, 120)],
    "top": [(30, -50), (150, -20), (170, 70), (60, 90)],
    "bottom": [(40, 110), (160, 130), (150, 260), (20, 230)],
}


def _exact_inside(poly, size):
    """Even-odd point-in-polygon at every pixel centre, in exact integer arithmetic: the crossings of the ray towards +x."""
    v = np.asarray(poly, np.int64).reshape(-1, 2)
    py, px = np.mgrid[0:size, 0:size].astype(np.int64)
    inside = np.zeros((size, size), bool)
    for (x0, y0), (x1, y1) in zip(np.roll(v, 1, 0), v):
        if y0 == y1:
            continue
        spans = (y0 > py) != (y1 > py)
        lhs, rhs = (px - x0) * (y1 - y0), (py - y0) * (x1 - x0)           # px < x0 + (py - y0)(x1 - x0) / (y1 - y0)
        inside ^= spans & ((lhs < rhs) if y1 > y0 else (lhs > rhs))
    return inside


def _near_an_edge(poly, size):
    """True where some edge comes within 1 px (Chebyshev) of the pixel: the closed square [x-1, x+1] x [y-1, y+1] meets the closed
    segment (separating axes: x, y and the segment's normal), in exact integer arithmetic."""
    v = np.asarray(poly, np.int64).reshape(-1, 2)
    py, px = np.mgrid[0:size, 0:size].astype(np.int64)
    near = np.zeros((size, size), bool)
    for (x0, y0), (x1, y1) in zip(np.roll(v, 1, 0), v):
        box = (min(x0, x1) <= px + 1) & (max(x0, x1) >= px - 1) & (min(y0, y1) <= py + 1) & (max(y0, y1) >= py - 1)
        cr = [(x1 - x0) * (py + b - y0) - (y1 - y0) * (px + a - x0) for a in (-1, 1) for b in (-1, 1)]
        one_side = np.all([c > 0 for c in cr], 0) | np.all([c < 0 for c in cr], 0)
        near |= box & ~one_side
    return near


@pytest.mark.parametrize("name", list(POLYGONS))
def test_fill_rule_against_exact_and_pillow(name):
    from PIL import Image, ImageDraw
    poly = np.asarray(POLYGONS[name], np.int32)
    assert (poly.max(0) - poly.min(0)).min() >= 64
    got = P.fill_mask([poly], CANVAS)
    exact = _exact_inside(poly, CANVAS)
    img = Image.new("L", (CANVAS, CANVAS), 0)
    ImageDraw.Draw(img).polygon([(int(x), int(y)) for x, y in poly], fill=1, outline=1)
    pillow = np.asarray(img) != 0
    far = ~_near_an_edge(poly, CANVAS)
    assert exact.sum() > 1000
    assert (exact & ~far).sum() <= 0.30 * exact.sum(), "the excluded band holds too much of the polygon to judge it"
    assert np.array_equal(got[far], exact[far]), int((got[far] != exact[far]).sum())
    assert np.array_equal(got[far], pillow[far]), int((got[far] != pillow[far]).sum())
    for x, y in poly:
        if 0 <= x < CANVAS and 0 <= y < CANVAS:
            assert got[y, x], (x, y)


def _mask_of(pixels, size):
    m = np.zeros((size, size), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def test_degenerate_contours_match_hand_written_masks():
    S = 16
    assert np.array_equal(P.fill_mask([[(5, 7)]], S), _mask_of([(5, 7)], S))                                    # 1 vertex
    assert np.array_equal(P.fill_mask([[(2, 3), (6, 3)]], S), _mask_of([(x, 3) for x in range(2, 7)], S))        # 2 vertices, horizontal
    assert np.array_equal(P.fill_mask([[(1, 1), (4, 4)]], S), _mask_of([(k, k) for k in range(1, 5)], S))        # 2 vertices, diagonal
    assert np.array_equal(P.fill_mask([[(3, 12), (3, 5)]], S), _mask_of([(3, y) for y in range(5, 13)], S))      # 2 vertices, vertical
    assert np.array_equal(P.fill_mask([[(1, 1), (3, 3), (6, 6)]], S), _mask_of([(k, k) for k in range(1, 7)], S))   # collinear
    assert np.array_equal(P.fill_mask([[(2, 2), (8, 2), (5, 2)]], S), _mask_of([(x, 2) for x in range(2, 9)], S))   # zero area
    assert np.array_equal(P.fill_mask([[(4, 4), (4, 9), (4, 4), (4, 9)]], S), _mask_of([(4, y) for y in range(4, 10)], S))
    for outside in ([(-10, -10), (-5, -3), (-2, -20)], [(20, 3), (30, 5), (25, 12)], [(2, 16), (9, 40), (5, 17)], [(3, -1), (12, -1)]):
        assert not P.fill_mask([outside], S).any(), outside
    # a vertex at x = C: the top edge and the fill stop at column 15; clipLine moves the hypotenuse's end from (16, 2) to (15, 3)
    want = _mask_of([(x, 2) for x in range(12, 16)] + [(x, 3) for x in range(12, 16)] + [(x, 4) for x in range(12, 15)] +
                    [(12, 5), (13, 5), (12, 6)], S)
    assert np.array_equal(P.fill_mask([[(16, 2), (12, 2), (12, 6)]], S), want)
    # the union of contours, and an axis-aligned rectangle: both closed ends filled
    rect = _mask_of([(x, y) for x in range(3, 9) for y in range(2, 6)], S)
    assert np.array_equal(P.fill_mask([[(3, 2), (8, 2), (8, 5), (3, 5)]], S), rect)
    assert np.array_equal(P.fill_mask([[(3, 2), (8, 2), (8, 5), (3, 5)], [(5, 7)]], S), rect | _mask_of([(5, 7)], S))
    assert not P.fill_mask([], S).any()


def test_line_iterator_reaches_both_ends_and_is_8_connected():
    rs = np.random.RandomState(1)
    for _ in range(200):
        (x0, y0), (x1, y1) = rs.randint(0, 40, (2, 2))
        px = P.line_pixels(40, (x0, y0), (x1, y1))
        assert len(px) == max(abs(x1 - x0), abs(y1 - y0)) + 1
        assert {px[0], px[-1]} == {(x0, y0), (x1, y1)}
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(px, px[1:]))
    for _ in range(200):                                                   # clipped: every pixel inside, none when the segment misses
        (x0, y0), (x1, y1) = rs.randint(-60, 100, (2, 2))
        assert all(0 <= x < 40 and 0 <= y < 40 for x, y in P.line_pixels(40, (x0, y0), (x1, y1)))


def test_pack_bits_layout():
    m = np.zeros((2, 40), bool)
    m[0, 0] = m[0, 31] = m[1, 32] = m[1, 39] = True
    assert np.array_equal(P.pack_bits(m), np.array([[0x80000001, 0], [0, 0x81]], np.uint32))


def test_paste_canvas_is_the_reference_expression():
    rs = np.random.RandomState(2)
    im = rs.randint(0, 256, (12, 12, 3)).astype(np.uint8)
    mask = rs.rand(12, 12) < 0.3
    want = im.copy()
    im_new = np.repeat(mask[..., None], 3, -1).astype(np.uint8)
    i = im_new[:, ::-1].astype(bool)                                      # cv2.flip(im_new, 1).astype(bool)
    want[i] = im[:, ::-1][i]                                               # im[i] = cv2.flip(im, 1)[i]
    assert np.array_equal(P.paste_canvas(im, mask), want)


# ---------------------------------------------------------------- opt-in and validation

def test_opt_in_and_validation():
    lab = [np.array([[1, 0.5, 0.5, 0.2, 0.2]], np.float32)]
    tri = np.array([[0.4, 0.4], [0.6, 0.4], [0.5, 0.6]], np.float32)
    with pytest.raises(M.MafError, match="polygon"):
        A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[tri]])
    with pytest.raises(M.MafError, match="polygon"):
        A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[tri]], polygons=False)
    A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[tri]], polygons=True)
    with pytest.raises(M.MafError):
        A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[tri, tri]], polygons=True)            # 2 polygons, 1 row
    with pytest.raises(M.MafError):
        A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[]], polygons=True)                    # a box row without a polygon
    with pytest.raises(M.MafError):
        A.TrainAugment(lab, [(10, 10)], HYP_N, segments=[[tri.reshape(-1)]], polygons=True)
    empty = [np.zeros((0, 5), np.float32)]
    A.TrainAugment(empty, [(10, 10)], HYP_N, segments=[[]], polygons=True)
    A.TrainAugment(empty, [(10, 10)], HYP_N, segments=[[]])
    aug = A.TrainAugment(empty, [(10, 10)], HYP_N, 64, segments=[[]], polygons=True)
    random.seed(0)
    np.random.seed(0)
    smp = aug.draw(0)
    assert all(layer.paste == [] for layer in smp.layers) and len(smp.labels) == 0


def test_polygons_without_segments_draw_like_boxes():
    """An image set without labels consumes the same random stream with and without polygons=True (copy_paste draws nothing)."""
    labels, shapes = [np.zeros((0, 5), np.float32)] * 3, [(20, 30), (64, 64), (50, 40)]
    out = []
    for polygons in (False, True):
        aug = A.TrainAugment(labels, shapes, HYP_N, 64, segments=[[], [], []], polygons=polygons)
        random.seed(5)
        np.random.seed(5)
        smp = aug.draw_batch([0, 1, 2, 1])
        out.append(([l.M for s in smp for l in s.layers], random.random()))
    assert out[0][1] == out[1][1] and all(np.array_equal(a, b) for a, b in zip(out[0][0], out[1][0]))


# ---------------------------------------------------------------- boundary (no device touched)

def test_library_declares_the_symbols():
    assert {"maf_polygon_mask", "maf_mosaic_affine_paste", "maf_augment_paste_size"} <= set(lib.EXPORTS)
    L = lib.load()
    assert L.maf_augment_paste_size() == C.sizeof(lib.MafAugmentPaste)


def _table(masks):
    tab, (n, npoly, nvert) = P.polygon_table(masks)
    return tab, n, npoly, nvert


def test_polygon_mask_rejects_bad_tables_before_the_device():
    L = lib.load()
    dev = C.c_void_p(64)                                                   # never dereferenced: validation fails first
    tab, n, npoly, nvert = _table([[[(1, 1), (5, 1), (3, 4)]], []])

    def call(t, n, npoly, nvert, size=64, out=dev, tab_dev=dev):
        return L.maf_polygon_mask(t.ctypes.data_as(C.c_void_p) if t is not None else None, tab_dev, n, npoly, nvert, size, out, None)
    with pytest.raises(M.MafError, match="null"):
        lib.check(call(None, n, npoly, nvert))
    with pytest.raises(M.MafError, match="null"):
        lib.check(call(tab, n, npoly, nvert, out=None))                    # a null mask with polygons
    with pytest.raises(M.MafError, match="null"):
        lib.check(call(tab, n, npoly, nvert, tab_dev=None))
    bad = tab.copy()
    bad[1], bad[2] = 1, 0                                                  # mask ranges out of order
    with pytest.raises(M.MafError, match="mask_start"):
        lib.check(call(bad, n, npoly, nvert))
    bad = tab.copy()
    bad[n + 1 + 1] = 5                                                     # polygon offsets past the vertices / out of order
    with pytest.raises(M.MafError, match="poly_start"):
        lib.check(call(bad, n, npoly, nvert))
    bad, _, _, _ = _table([[[(1, 1), (5, 1)], [(2, 2)]]])
    bad[1 + 1 + 1] = 3                                                     # offsets 0, 3, 3: not strictly rising (an empty contour)
    with pytest.raises(M.MafError, match="poly_start"):
        lib.check(call(bad, 1, 2, 3))
    bad = tab.copy()
    bad[-1] = P.COORD_MAX + 1                                              # a vertex out of the validated range
    with pytest.raises(M.MafError, match="vertex"):
        lib.check(call(bad, n, npoly, nvert))
    bad[-1] = -P.COORD_MAX - 2
    with pytest.raises(M.MafError, match="vertex"):
        lib.check(call(bad, n, npoly, nvert))
    with pytest.raises(M.MafError, match="C must"):
        lib.check(call(tab, n, npoly, nvert, size=0))
    with pytest.raises(M.MafError, match="n must"):
        lib.check(call(tab, 0, npoly, nvert))


def test_mosaic_affine_paste_rejects_bad_arguments_before_the_device():
    L = lib.load()
    s = lib.MafAugmentSample()
    p = lib.MafAugmentPaste()
    dev = C.c_void_p(64)
    s.ntiles[0] = 1
    t = s.tile[0][0]
    t.ptr, t.pitch, t.w, t.h = 64, 30, 10, 10
    t.x0, t.y0, t.x1, t.y1, t.dx, t.dy = 0, 0, 10, 10, 0, 0
    p.C = 128
    with pytest.raises(M.MafError, match="null"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, None, None, 1, 64, dev, None))
    with pytest.raises(M.MafError, match="null"):
        lib.check(L.maf_mosaic_affine_paste(None, None, C.byref(p), dev, 1, 64, dev, None))
    p.mask[0] = 64
    p.C = 100                                                              # C is not 2 S
    with pytest.raises(M.MafError, match="2 S"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, C.byref(p), dev, 1, 64, dev, None))
    p.C = 128
    p.mask[0] = 66                                                         # masks are 32-bit words
    with pytest.raises(M.MafError, match="aligned"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, C.byref(p), dev, 1, 64, dev, None))
    p.mask[0], p.mask[1] = 0, 64                                           # a mask for a layer that does not exist
    with pytest.raises(M.MafError, match="layer"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, C.byref(p), dev, 1, 64, dev, None))
    p.mask[0], p.mask[1] = 64, 0
    t.x1 = 11                                                              # the sample table is checked as maf_mosaic_affine checks it
    with pytest.raises(M.MafError, match="outside"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, C.byref(p), dev, 1, 64, dev, None))
    t.x1 = 10
    with pytest.raises(M.MafError, match="multiple of 32"):
        lib.check(L.maf_mosaic_affine_paste(C.byref(s), dev, C.byref(p), dev, 1, 100, dev, None))


def test_train_batch_with_polygons_has_no_cpu_fallback():
    tri = np.array([[0.2, 0.2], [0.8, 0.3], [0.5, 0.9]], np.float32)
    lab = np.array([[1, 0.5, 0.55, 0.6, 0.7]], np.float32)
    aug = A.TrainAugment([lab], [(8, 8)], dict(HYP_N, copy_paste=1.0), 64, segments=[[tri]], polygons=True)
    with pytest.raises(M.MafError, match="CUDA"):
        M.train_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], [0], aug)


def test_torch_ops_fake_kernels():
    from maf_yolo_amd import torch_ops
    ops = torch_ops.load()
    assert hasattr(ops, "polygon_mask") and hasattr(ops, "mosaic_affine_paste")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        tab = torch.empty(3, C.sizeof(lib.MafAugmentSample), dtype=torch.uint8)
        paste = torch.empty(3, C.sizeof(lib.MafAugmentPaste), dtype=torch.uint8)
        out = ops.mosaic_affine_paste(tab, tab.to("cuda"), paste, paste.to("cuda"), 640)
        assert tuple(out.shape) == (3, 3, 640, 640) and out.dtype == torch.uint8
        pt = torch.empty(20, dtype=torch.int32)
        masks = ops.polygon_mask(pt, pt.to("cuda"), 2, 1, 3, 100)
        assert tuple(masks.shape) == (2, 100, 4) and masks.dtype == torch.int32
