"""-m gpu: the letterbox layer on the device (csrc/letterbox.hip, maf-yolo_amd/letterbox.py).

* the kernel equals the NumPy restatement of OpenCV's uint8 INTER_LINEAR (tests/letterbox_ref.py) bit for bit: 1080p (3x linear), 720p (2x
  area-fast), 480 x 640 (pad only), 333 x 500 (eval-mode upscale), 17 x 1000, 1 x 1, rows that are not 16-byte multiples, cropped views, BGR
  and RGB, auto on and off, a non-grey colour, mixed batches up to B = 64 and past the kernel-argument table (device table);
* rescale_boxes equals the reference's Inferer.rescale(...).round() (tests/golden/letterbox_cases.npz) for the three result forms;
* detect_frames / eval_batch end to end against the path that exists without them;
* no host synchronisation except detect_frames' one count copy.
"""
import importlib

import numpy as np
import pytest
import torch

import letterbox_ref as R
import maf_yolo_amd as M
from oracle import maf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LB = importlib.import_module("maf_yolo_amd.letterbox")


def _frames(sizes, seed=0):
    host = [R.synth_frame(h, w, seed + i) for i, (h, w) in enumerate(sizes)]
    return host, [torch.from_numpy(f).to(DEV) for f in host]


def _want(host, new_shape=640, color=(114, 114, 114), auto=True, scaleup=True, stride=32, bgr=True):
    ns = LB.check_img_size(new_shape if isinstance(new_shape, int) else list(new_shape), stride)
    out = []
    for f in host:
        g = LB.letterbox_geometry(f.shape[0], f.shape[1], tuple(ns), auto, scaleup, stride)
        out.append(R.letterbox_pixels(f, g["new_unpad"], g["top"], g["left"], g["shape"][0], g["shape"][1], color, bgr))
    return np.stack(out)


@pytest.mark.parametrize("sizes,auto", [
    ([(1080, 1920)] * 2, True),
    ([(720, 1280)] * 2, True),
    ([(480, 640)], True),
    ([(333, 500)], False),
    ([(17, 1000)], True),
    ([(1, 1)], False),
    ([(1080, 1920), (720, 1280), (480, 640), (333, 500), (17, 1000), (1, 1), (101, 77), (500, 333)], False),
])
@pytest.mark.parametrize("bgr", [True, False])
def test_letterbox_equals_restatement(sizes, auto, bgr):
    host, dev = _frames(sizes, 3)
    color = (114, 114, 114) if bgr else (7, 200, 33)
    imgs, ratios, pads = M.letterbox(dev, 640, color=color, auto=auto, bgr=bgr)
    want = _want(host, 640, color, auto, True, 32, bgr)
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == want.shape
    assert np.array_equal(imgs.cpu().numpy(), want)
    g = LB.letterbox_geometry(sizes[0][0], sizes[0][1], (640, 640), auto, True, 32)
    assert ratios[0] == g["ret"][0] and pads[0] == g["ret"][1]


def test_letterbox_border_is_the_colour_and_views_with_pitch():
    host, dev = _frames([(1080, 1920)], 5)
    big = torch.from_numpy(host[0]).to(DEV)
    crops = [big[3:720, 5:1283], big[1:334, 1:501], big[0:17, 1:1001], big[7:8, 9:10], big[2:100, 3:50],
             big[1:321, 3:323]]                                    # pitch 5760 > 3 w, odd offsets; the last one is a copy (320 x 320 at 320)
    cpu = [c.cpu().numpy() for c in crops]
    color = (10, 20, 30)
    imgs, _, _ = M.letterbox(crops, 320, color=color, auto=False)
    want = _want(cpu, 320, color, False)
    assert np.array_equal(imgs.cpu().numpy(), want)
    g = LB.letterbox_geometry(717, 1278, (320, 320), False, True, 32)
    top = g["top"]
    assert top > 0 and (imgs[0, :, :top] == torch.tensor([30, 20, 10], device=DEV, dtype=torch.uint8).view(3, 1, 1)).all()


def test_letterbox_batch_tensor_scaleup_off_and_stride64():
    host, _ = _frames([(333, 500)] * 3, 9)
    x = torch.from_numpy(np.stack(host)).to(DEV)
    imgs, _, _ = M.letterbox(x, (384, 640), scaleup=False, stride=64)
    assert np.array_equal(imgs.cpu().numpy(), _want(host, (384, 640), scaleup=False, stride=64))


@pytest.mark.parametrize("B", [64, 70])
def test_letterbox_large_mixed_batches(B):
    rs = np.random.RandomState(B)
    sizes = [(int(rs.randint(1, 700)), int(rs.randint(1, 700))) for _ in range(B)]
    host, dev = _frames(sizes, 100)
    imgs, _, _ = M.letterbox(dev, 320, auto=False)                 # B = 70: the table goes to the device (past MAF_LETTERBOX_KARG_MAX)
    assert np.array_equal(imgs.cpu().numpy(), _want(host, 320, auto=False))


def test_eval_batch_equals_restatement_and_shapes():
    sizes = [(333, 500), (480, 640), (375, 500), (640, 427)]
    host, dev = _frames(sizes, 21)
    imgs, shapes = M.eval_batch(dev)
    bs = LB.rect_batch_shape(sizes)
    want = []
    for f in host:
        g = LB.eval_geometry(f.shape[0], f.shape[1], bs)
        want.append(R.letterbox_pixels(f, g["new_unpad"], g["top"], g["left"], bs[0], bs[1]))
        assert shapes[len(want) - 1] == g["shapes"]
    assert np.array_equal(imgs.cpu().numpy(), np.stack(want))


def test_mixed_auto_batch_raises():
    _, dev = _frames([(1080, 1920), (480, 640)])
    with pytest.raises(ValueError, match="different shapes"):
        M.letterbox(dev, 640)


def test_non_uint8_frames_raise():
    with pytest.raises(M.MafError):
        M.letterbox([torch.zeros(8, 8, 3, device=DEV)])


# ---------------------------------------------------------------- rescale

def _rescale_cases(golden):
    z = golden("letterbox_cases")
    off, out = 0, []
    for H, W, h0, w0, n in z["rescale_meta"]:
        out.append(((int(H), int(W)), (int(h0), int(w0)), z["rescale_in"][off:off + n], z["rescale_out"][off:off + n]))
        off += n
    return out


def test_rescale_boxes_equals_reference_all_forms(golden):
    cases = _rescale_cases(golden)
    for (H, W), (h0, w0), bin_, bout in cases:
        n = bin_.shape[0]
        # list form
        dets = [torch.from_numpy(bin_.copy()).to(DEV)]
        M.rescale_boxes(dets, (H, W), [(h0, w0)])
        assert np.array_equal(dets[0].cpu().numpy(), bout)
        # (rows, idx, count) triple with max_det > n
        rows = torch.zeros(1, n + 5, 6, device=DEV)
        rows[0, :n] = torch.from_numpy(bin_).to(DEV)
        rows[0, n:] = 12345.0
        cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
        M.rescale_boxes((rows, None, cnt), (H, W), [(h0, w0)])
        assert np.array_equal(rows[0, :n].cpu().numpy(), bout) and (rows[0, n:] == 12345.0).all()
    # NmsHandle form: a whole batch at once
    B = len(cases)
    md = max(c[2].shape[0] for c in cases) + 1
    for (H, W) in {c[0] for c in cases}:
        sel = [c for c in cases if c[0] == (H, W)]
        rows = torch.zeros(len(sel), md, 6, device=DEV)
        for b, c in enumerate(sel):
            rows[b, :c[2].shape[0]] = torch.from_numpy(c[2]).to(DEV)
        cnt = torch.tensor([c[2].shape[0] for c in sel], dtype=torch.int32, device=DEV)
        ev = torch.cuda.Event()
        ev.record()
        h = M.nms.NmsHandle(rows, None, cnt, ev)
        M.rescale_boxes(h, (H, W), [c[1] for c in sel])
        for b, c in enumerate(sel):
            assert np.array_equal(rows[b, :c[2].shape[0]].cpu().numpy(), c[3])
    assert B >= 5


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def model_n():
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0))
    return m.to(DEV).eval()


def test_detect_frames_equals_existing_path(model_n):
    sizes = [(1080, 1920), (720, 1280), (480, 640), (333, 500)]
    host, dev = _frames(sizes, 40)
    dets = M.detect_frames(model_n, dev, 640, conf_thres=0.03, iou_thres=0.45, auto=False)
    x = torch.from_numpy(_want(host, 640, auto=False)).to(DEV)     # the restatement's batch through the existing path
    with torch.no_grad():
        pred = model_n(x)[0]
    ref = M.non_max_suppression(pred, 0.03, 0.45, max_det=1000)
    assert [d.shape[0] for d in dets] == [r.shape[0] for r in ref]
    assert sum(d.shape[0] for d in dets) > 0
    for d, r, (h0, w0) in zip(dets, ref, sizes):
        want = r.cpu().numpy().copy()
        want[:, :4] = R.rescale((640, 640), want[:, :4], (h0, w0))[:, :4]
        assert np.array_equal(d.cpu().numpy(), want)


def test_detect_frames_auto_same_aspect(model_n):
    sizes = [(1080, 1920), (720, 1280)]                            # both letterbox to 384 x 640 with auto=True
    host, dev = _frames(sizes, 50)
    dets = M.detect_frames(model_n, dev, 640, conf_thres=0.03)
    x = torch.from_numpy(_want(host, 640)).to(DEV)
    assert tuple(x.shape[2:]) == (384, 640)
    with torch.no_grad():
        ref = M.non_max_suppression(model_n(x)[0], 0.03, 0.45, max_det=1000)
    for d, r, (h0, w0) in zip(dets, ref, sizes):
        want = r.cpu().numpy().copy()
        want[:, :4] = R.rescale((384, 640), want[:, :4], (h0, w0))[:, :4]
        assert np.array_equal(d.cpu().numpy(), want)


def test_eval_batch_to_coco_rows(model_n):
    sizes = [(480, 640), (333, 500), (640, 427)]
    _, dev = _frames(sizes, 60)
    imgs, shapes = M.eval_batch(dev)
    with torch.no_grad():
        pred = model_n(imgs)[0]
    raw = M.nms_raw(pred, 0.03, 0.65, multi_label=True)
    ids = list(range(1, 81))
    res = M.convert_to_coco_format(raw, imgs, ["1.jpg", "2.jpg", "3.jpg"], shapes, ids)
    counts = raw[2].tolist()
    outs = [raw[0][b, :n].cpu().numpy() for b, n in enumerate(counts)]
    iid, cid, bb, sc = O.coco_rows(outs, shapes, [1, 2, 3], ids)
    assert len(res) == sum(counts) > 0 and [r["image_id"] for r in res] == iid.tolist() and [r["category_id"] for r in res] == cid.tolist()
    assert np.array_equal(np.asarray([r["bbox"] for r in res]).reshape(-1, 4), bb) and np.array_equal(np.asarray([r["score"] for r in res]), sc)


def test_no_host_sync(model_n, monkeypatch):
    _, dev = _frames([(1080, 1920), (720, 1280)], 70)
    _, dev70 = _frames([(50, 60)] * 70, 80)
    M.letterbox(dev, 640)                                         # warm: op library loaded, pinned pool primed, the model's plan built
    M.detect_frames(model_n, dev, 640)
    torch.cuda.synchronize()
    # detect_frames' one documented sync is the copy of the NMS counts: that copy alone runs with the sync check off, everything before and
    # after it (letterbox, forward, nms_raw, the rescale, the slicing of the result) runs under "error"
    copies = []
    real_nms_raw = LB.nms_raw

    def nms_raw(*a, **k):
        rows, idx, cnt = real_nms_raw(*a, **k)

        def tolist():
            torch.cuda.set_sync_debug_mode(0)
            try:
                copies.append(torch.Tensor.tolist(cnt))
            finally:
                torch.cuda.set_sync_debug_mode("error")
            return copies[-1]
        cnt.tolist = tolist
        return rows, idx, cnt

    monkeypatch.setattr(LB, "nms_raw", nms_raw)
    torch.cuda.set_sync_debug_mode("error")
    try:
        imgs, _, _ = M.letterbox(dev, 640)
        M.letterbox(dev70, 320, auto=False)
        M.eval_batch([d[:300, :600] for d in dev])
        rows = torch.zeros(2, 10, 6, device=DEV)
        cnt = torch.full((2,), 3, dtype=torch.int32, device=DEV)
        M.rescale_boxes((rows, None, cnt), (384, 640), [(1080, 1920), (720, 1280)])
        M.rescale_boxes([rows[0, :3].clone(), rows[1, :2].clone()], (384, 640), [(1080, 1920), (720, 1280)])
        dets = M.detect_frames(model_n, dev, 640)
        with pytest.raises(RuntimeError):                         # the check is live: an unguarded count copy raises
            torch.Tensor.tolist(cnt)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert len(copies) == 1 and [d.shape[0] for d in dets] == copies[0]
