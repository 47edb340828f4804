"""-m gpu: copy_paste on polygon labels on the device (csrc/polygon_mask.hip, maf_mosaic_affine_paste in csrc/augment.hip,
maf-yolo_amd/augment.py TrainAugment(polygons=True)), through the C-ABI.

* maf_polygon_mask equals the restatement's fill_mask (tests/copy_paste_ref.py) bit for bit: contours across the 31/32 word boundary and
  the 8-row band boundary, clipped at all four borders, the degenerate set, a bow-tie, 300 vertices, 0 / 1 / 40 contours per mask, 5 masks
  in one launch into a buffer pre-filled with 0xFF, a canvas that is no multiple of 32, and a 1280 canvas;
* train_batch with polygons equals the restatement bit for bit (pasted contours in both layers, and the paste changes pixels);
* a batch without pasted contours takes the maf_mosaic_affine path, and maf_mosaic_affine_paste without masks gives its bytes;
* the torch ops and the C-ABI agree; bad tables are rejected with the error code before any launch; no device -> host synchronisation.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import augment_ref as R
import copy_paste_ref as P
import maf_yolo_amd as M
from maf_yolo_amd import augment as A
from maf_yolo_amd import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYP_N = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
             mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)
HYP_M = dict(HYP_N, copy_paste=0.2, mixup=0.1, dy_mixup=0.4)
HYPS = {"m": HYP_M, "stress": dict(HYP_M, copy_paste=1.0, degrees=5.0, shear=2.0)}
E_ARG = -1                                     # MAF_E_ARG (include/mafyolo_hip.h)
SIZES = [(48, 64), (64, 64), (77, 61), (108, 192), (30, 20), (72, 128), (63, 17), (128, 128), (33, 50), (61, 45), (17, 63), (96, 64)]


# ---------------------------------------------------------------- maf_polygon_mask

def _run_polygon_mask(masks, size):
    tab, (n, npoly, nvert) = P.polygon_table(masks)
    W = (size + 31) // 32
    out = torch.full((n, size, W), -1, dtype=torch.int32, device=DEV)                       # 0xFF everywhere: every word must be written
    tab_dev = torch.from_numpy(tab).to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    lib.check(lib.load().maf_polygon_mask(tab.ctypes.data, tab_dev.data_ptr(), n, npoly, nvert, size, out.data_ptr(), st))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _blob(size, nv=300):
    rs = np.random.RandomState(3)
    t = np.linspace(0, 2 * np.pi, nv, endpoint=False)
    r = size * (0.32 + 0.05 * np.sin(5 * t)) + rs.uniform(-1.5, 1.5, nv)
    return np.stack([size / 2 + r * np.cos(t), size / 2 + r * np.sin(t)], 1).round().astype(np.int32)


def _cases(size):
    S = size
    rs = np.random.RandomState(size)
    degenerate = [[(5, 7)], [(2, 3), (40, 3)], [(1, 1), (44, 44)], [(3, 30), (3, 5)], [(1, 1), (13, 13), (36, 36)], [(2, 20), (38, 20), (15, 20)],
                  [(-10, -10), (-5, -3), (-2, -20)], [(S + 4, 3), (S + 30, 5), (S + 9, 12)], [(3, -1), (12, -1)],
                  [(S, 2), (S - 4, 2), (S - 4, 6)], [(S - 1, S - 1)], [(0, 0), (S, S)]]
    borders = [[(-S // 2, 10), (S // 2, 14), (S // 3, S - 9), (-S // 3, S - 20)],                     # left
               [(S - 20, 5), (2 * S, 11), (S + S // 2, S - 6), (S - 9, S - 30)],                      # right
               [(9, -S // 2), (S - 9, -7), (S - 14, 21), (20, 30)],                                   # top
               [(12, S - 21), (S - 7, S - 15), (S - 14, 2 * S), (5, S + 9)],                          # bottom
               [(-30000, -20000), (32767, -32767), (S // 2, S // 2)]]                                 # the whole validated range
    random40 = []
    for _ in range(40):
        k = int(rs.randint(1, 9))
        c = rs.randint(-8, S + 8, 2)
        random40.append((c + rs.randint(-S // 3, S // 3 + 1, (k, 2))).astype(np.int32))
    return [
        [[(20, 3), (45, 6), (37, 13), (25, 10)]],                                                     # 1 contour: bits 31 / 32, rows 7 / 8
        borders,
        [],                                                                                           # 0 contours
        degenerate + [[(4, 4), (S - 6, S - 9), (S - 6, 4), (4, S - 9)], _blob(S),                      # a bow-tie, 300 vertices
                      [(31, 7), (32, 7), (32, 8), (31, 8)], [(28, 15), (35, 15), (35, 16), (28, 16)], [(0, 7), (S - 1, 8)], [(31, 0), (32, S - 1)]],
        random40,
    ]


@pytest.mark.parametrize("size", [64, 128, 50])
def test_polygon_mask_equals_fill_mask(size):
    masks = _cases(size)
    assert [len(m) for m in masks][:3] == [1, 5, 0] and len(masks[4]) == 40 and len(masks) == 5
    got = _run_polygon_mask(masks, size)
    for i, m in enumerate(masks):
        want = P.pack_bits(P.fill_mask(m, size))
        assert np.array_equal(got[i], want), (size, i, int((got[i] != want).sum()))
    assert not got[2].any()
    for i, m in enumerate(masks):                                                                     # contour by contour: which one differs
        if i in (1, 3):
            each = _run_polygon_mask([[p] for p in m], size)
            for k, p in enumerate(m):
                assert np.array_equal(each[k], P.pack_bits(P.fill_one(p, size))), (size, i, k)


def test_polygon_mask_canvas_1280():
    polys = [[(100, 90), (1190, 160), (1260, 1100), (640, 1275), (30, 700)], [(-200, 500), (400, 300), (700, 1500), (90, 1400)], _blob(1280)]
    got = _run_polygon_mask([polys], 1280)
    want = P.pack_bits(P.fill_mask(polys, 1280))
    assert np.array_equal(got[0], want), int((got[0] != want).sum())


def test_polygon_mask_torch_op_and_c_abi_agree():
    from maf_yolo_amd import torch_ops
    masks = _cases(128)
    tab, (n, npoly, nvert) = P.polygon_table(masks)
    t = torch.from_numpy(tab)
    via_op = torch_ops.load().polygon_mask(t, t.to(DEV), n, npoly, nvert, 128)
    assert via_op.dtype == torch.int32 and tuple(via_op.shape) == (5, 128, 4) and via_op.device == DEV
    assert np.array_equal(via_op.cpu().numpy().view(np.uint32), _run_polygon_mask(masks, 128))


def test_bad_tables_are_rejected_before_any_launch():
    L = lib.load()
    masks = [[[(1, 1), (50, 1), (30, 40)], [(5, 5), (9, 9)]], []]
    tab, (n, npoly, nvert) = P.polygon_table(masks)
    out = torch.full((n, 64, 2), -1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    kept = []                                                                                         # device copies stay alive to the end

    def rc(t, out_ptr=out.data_ptr(), size=64):
        t_dev = torch.from_numpy(t).to(DEV)
        kept.append(t_dev)
        return L.maf_polygon_mask(t.ctypes.data, t_dev.data_ptr(), n, npoly, nvert, size, out_ptr, st)
    assert rc(tab, out_ptr=None) == E_ARG                                                         # a null mask with polygons
    bad = tab.copy()
    bad[n + 1 + 1], bad[n + 1 + 2] = 5, 3                                                             # offsets out of order
    assert rc(bad) == E_ARG
    bad = tab.copy()
    bad[1], bad[2] = 2, 1                                                                             # mask ranges out of order
    assert rc(bad) == E_ARG
    for v in (P.COORD_MAX + 1, -P.COORD_MAX - 1, 2 ** 31 - 1, -2 ** 31):                              # vertices out of the validated range
        bad = tab.copy()
        bad[-2] = v
        assert rc(bad) == E_ARG
    assert rc(tab, size=0) == E_ARG and rc(tab, size=16385) == E_ARG
    with pytest.raises(M.MafError, match="vertex"):
        lib.check(rc(bad))
    torch.cuda.synchronize()
    assert (out == -1).all(), "a rejected call launched"
    from maf_yolo_amd import torch_ops
    t = torch.from_numpy(tab)
    with pytest.raises(RuntimeError, match="CPU"):
        torch_ops.load().polygon_mask(t, t, n, npoly, nvert, 64)                                     # CPU tensors: no CPU path
    with pytest.raises(RuntimeError, match="CPU int32"):
        torch_ops.load().polygon_mask(t.to(DEV), t.to(DEV), n, npoly, nvert, 64)                     # the table to validate stays on the host


# ---------------------------------------------------------------- train_batch with polygons

def _dataset(seed, n_img=16):
    """Frames of odd sizes (some as cropped views with a row pitch) with 1..5 seeded polygons each and the box labels derived from them."""
    rs = np.random.RandomState(seed)
    sizes = list(SIZES)
    while len(sizes) < n_img:
        sizes.append((int(rs.randint(16, 160)), int(rs.randint(16, 160))))
    labels, segments = [], []
    for _ in sizes:
        segs, rows = [], []
        for _ in range(int(rs.randint(1, 6))):
            k = int(rs.randint(3, 10))
            c, rad = rs.uniform(0.15, 0.85, 2), rs.uniform(0.05, 0.3, 2)
            ang = np.sort(rs.uniform(0, 2 * np.pi, k))
            xy = np.stack([c[0] + rad[0] * np.cos(ang), c[1] + rad[1] * np.sin(ang)], 1).clip(0, 1).astype(np.float32)
            segs.append(xy)
            lo, hi = xy.min(0), xy.max(0)
            rows.append([float(rs.randint(0, 80)), (lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[0] - lo[0], hi[1] - lo[1]])
        segments.append(segs)
        labels.append(np.array(rows, np.float32).reshape(-1, 5))
    host = [R.synth_frame(h, w, seed * 100 + i) for i, (h, w) in enumerate(sizes)]
    frames = []
    for i, f in enumerate(host):
        if i % 3 == 1:
            big = np.zeros((f.shape[0] + 3, f.shape[1] + 5, 3), np.uint8)
            big[2:2 + f.shape[0], 3:3 + f.shape[1]] = f
            frames.append(torch.from_numpy(big).to(DEV)[2:2 + f.shape[0], 3:3 + f.shape[1]])
        else:
            frames.append(torch.from_numpy(f).to(DEV))
    return sizes, labels, segments, host, frames


def _draw(aug, B, seed):
    random.seed(seed)
    np.random.seed(seed)
    return aug.draw_batch(np.random.RandomState(seed).randint(0, len(aug), B))


def _want(aug, samples, host, paste=True):
    staged = R.staged_frames(aug, samples, dict(enumerate(host)))
    return np.stack([P.sample_pixels(aug, smp, staged, paste) for smp in samples])


def _check_batch(name, seed, img_size, B):
    sizes, labels, segments, host, frames = _dataset(seed)
    aug = A.TrainAugment(labels, sizes, HYPS[name], img_size, segments=segments, polygons=True)
    samples = _draw(aug, B, seed)
    imgs, targets = M.train_batch(frames, samples, aug)
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (B, 3, img_size, img_size) and imgs.device == DEV
    got = imgs.cpu().numpy()
    want = _want(aug, samples, host)
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (name, seed, b, int((got[b] != want[b]).sum()))
    rows = np.concatenate([np.concatenate([np.full((len(s.labels), 1), b, np.float32), s.labels.astype(np.float32)], 1) for b, s in
                           enumerate(samples)], 0).reshape(-1, 6)
    assert np.array_equal(targets.cpu().numpy(), rows)
    return aug, samples, host, got


@pytest.mark.parametrize("name", list(HYPS))
@pytest.mark.parametrize("seed", [2, 3, 4])
@pytest.mark.parametrize("img_size", [64, 96])
def test_train_batch_equals_restatement(name, seed, img_size):
    aug, samples, host, got = _check_batch(name, seed, img_size, 8)
    assert any(s.layers[0].paste for s in samples), "nothing was pasted in layer 0"
    assert any(len(s.layers) == 2 and s.layers[1].paste for s in samples), "nothing was pasted in layer 1"
    assert (got != _want(aug, samples, host, paste=False)).any(), "the paste changed no pixel"


def test_train_batch_640():
    aug, samples, host, got = _check_batch("stress", 4, 640, 2)
    assert any(layer.paste for s in samples for layer in s.layers)
    assert (got != _want(aug, samples, host, paste=False)).any()


def test_a_batch_without_paste_takes_the_plain_path(monkeypatch):
    sizes, labels, segments, host, frames = _dataset(5)
    aug = A.TrainAugment(labels, sizes, dict(HYP_M, copy_paste=0.0), 64, segments=segments, polygons=True)
    samples = _draw(aug, 8, 5)
    assert not any(layer.paste for s in samples for layer in s.layers) and A.stage_paste(samples) is None
    monkeypatch.setattr(A, "_mosaic_affine_paste", None)                                              # the plain path never reaches it
    imgs, _ = M.train_batch(frames, samples, aug)
    assert np.array_equal(imgs.cpu().numpy(), _want(aug, samples, host))
    # the same table through maf_mosaic_affine and, with a paste table without masks, through maf_mosaic_affine_paste
    table, dev, keep = A.stage_batch(frames, samples, aug)
    table_dev = table.to(DEV)
    ptab = (lib.MafAugmentPaste * 8)()
    for e in ptab:
        e.C = 128
    paste_dev = torch.from_numpy(np.frombuffer(ptab, np.uint8).copy()).to(DEV)
    a, b = (torch.full((8, 3, 64, 64), 7, dtype=torch.uint8, device=DEV) for _ in range(2))
    st = torch.cuda.current_stream(DEV).cuda_stream
    L = lib.load()
    lib.check(L.maf_mosaic_affine(table.data_ptr(), table_dev.data_ptr(), 8, 64, a.data_ptr(), st))
    lib.check(L.maf_mosaic_affine_paste(table.data_ptr(), table_dev.data_ptr(), C.addressof(ptab), paste_dev.data_ptr(), 8, 64, b.data_ptr(), st))
    torch.cuda.synchronize()
    del keep
    assert torch.equal(a, imgs) and torch.equal(b, imgs)


def test_paste_torch_op_c_abi_and_train_batch_agree():
    from maf_yolo_amd import torch_ops
    sizes, labels, segments, host, frames = _dataset(6)
    aug = A.TrainAugment(labels, sizes, HYPS["stress"], 64, segments=segments, polygons=True)
    samples = _draw(aug, 4, 6)
    via_batch, _ = M.train_batch(frames, samples, aug)
    table, dev, keep = A.stage_batch(frames, samples, aug)
    ptable, (n, npoly, nvert), slots = A.stage_paste(samples)
    assert n >= 2
    ops = torch_ops.load()
    pt = torch.from_numpy(ptable)
    masks = ops.polygon_mask(pt, pt.to(DEV), n, npoly, nvert, 128)
    ptab = (lib.MafAugmentPaste * 4)()
    for e in ptab:
        e.C = 128
    for i, (b, l) in enumerate(slots):
        ptab[b].mask[l] = masks[i].data_ptr()
    paste = torch.from_numpy(np.frombuffer(ptab, np.uint8).reshape(4, -1).copy())
    table_dev, paste_dev = table.to(DEV), paste.to(DEV)
    via_op = ops.mosaic_affine_paste(table, table_dev, paste, paste_dev, 64)
    via_abi = torch.empty(4, 3, 64, 64, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    L = lib.load()
    lib.check(L.maf_mosaic_affine_paste(table.data_ptr(), table_dev.data_ptr(), paste.data_ptr(), paste_dev.data_ptr(), 4, 64, via_abi.data_ptr(), st))
    # rejected before any launch: C that is not 2 S, and CPU tensors
    untouched = torch.full((4, 3, 64, 64), 9, dtype=torch.uint8, device=DEV)
    ptab[0].C = 64
    bad = torch.from_numpy(np.frombuffer(ptab, np.uint8).reshape(4, -1).copy())
    assert L.maf_mosaic_affine_paste(table.data_ptr(), table_dev.data_ptr(), bad.data_ptr(), paste_dev.data_ptr(), 4, 64, untouched.data_ptr(), st) == E_ARG
    with pytest.raises(RuntimeError, match="2 S"):
        ops.mosaic_affine_paste(table, table_dev, bad, paste_dev, 64)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.mosaic_affine_paste(table, table, paste, paste, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mosaic_affine_paste(table, table_dev, paste, paste, 64)
    torch.cuda.synchronize()
    del keep
    assert torch.equal(via_op, via_batch) and torch.equal(via_abi, via_batch) and (untouched == 9).all()
    with pytest.raises(M.MafError, match="CUDA"):
        M.train_batch([torch.from_numpy(f) for f in host], samples, aug)


def test_no_host_sync():
    sizes, labels, segments, host, frames = _dataset(7)
    aug = A.TrainAugment(labels, sizes, HYPS["stress"], 64, segments=segments, polygons=True)
    M.train_batch(frames, _draw(aug, 4, 7), aug)               # warm: op library loaded, pinned pool primed
    samples = _draw(aug, 8, 8)
    assert any(layer.paste for s in samples for layer in s.layers)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        imgs, targets = M.train_batch(frames, samples, aug)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert tuple(imgs.shape) == (8, 3, 64, 64) and targets.shape[1] == 6
