"""GPU tests of the in-process precision / recall / mAP (maf-yolo_amd/metrics.py over csrc/pr_metric.hip) against the NumPy restatement
(tests/pr_metric_ref.py) and the reference fixture (tests/golden/pr_metric_cases.npz): masks and confusion matrices bit for bit, curves
within 1e-12, the summary equal; degenerate inputs, device-side errors, EvalLoop end to end and the host-sync contract."""
import importlib
import warnings

import numpy as np
import pytest
import torch

import pr_metric_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import lib
from oracle import maf_oracle as O
from test_pr_metric_host import fixture_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EL = importlib.import_module("maf_yolo_amd.eval_loop")


def _pad(rows, max_det):
    out = np.zeros((rows.shape[0], max_det, 6), np.float32)
    out[:, :rows.shape[1]] = rows
    return out


def _feed(pm, batches, hw, se, max_det=300):
    for rows, count, targets, shapes in batches:
        pm.update(torch.from_numpy(_pad(rows, max_det)).to(DEV), torch.from_numpy(np.asarray(count, np.int32)).to(DEV),
                  torch.from_numpy(np.asarray(targets, np.float32).reshape(-1, 6)).to(DEV), hw, shapes, scale_exact=se)


def _records(pm):
    """(mask bits [n, niou], conf, cls) of every record, in sequence order."""
    n = int(pm.offs[pm.batches].item())
    keys = pm.keys[:n].cpu().numpy()
    m = pm.masks[:n].cpu().numpy().astype(np.int64) & 0xFFFF
    tp = ((m[:, None] >> np.arange(pm.niou)) & 1).astype(bool)
    u = (~keys & 0xFFFFFFFF).astype(np.uint32)
    bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32)
    return tp, bits.view(np.float32), (keys >> 32).astype(np.float64)


def _ref_tp(ref):
    parts = [s[0] for s in ref.stats if len(s[1])]
    return np.concatenate(parts, 0) if parts else np.zeros((0, 10), bool)


def _assert_same(res, want, name=""):
    assert res.seen == want["seen"], name
    assert np.array_equal(res.nt, want["nt"]), name
    if want["matrix"] is not None:
        assert np.array_equal(res.matrix, want["matrix"]), name
    assert res.pr_metric_result == (want["map50"], want["map"]) or np.allclose(res.pr_metric_result, (want["map50"], want["map"]),
                                                                                rtol=0, atol=1e-12), name
    if "p" not in want:
        assert not res.ok and res.pr_metric_result == (0.0, 0.0), name
        return
    for k in ("p", "r", "f1", "ap", "py"):
        np.testing.assert_allclose(getattr(res, k), want[k], rtol=0, atol=1e-12, err_msg="%s %s" % (name, k))
    assert res.f1_index == want["f1_index"], name
    assert np.array_equal(res.ap_class, want["ap_class"]), name
    np.testing.assert_allclose([res.mp, res.mr, res.mf1, res.map50, res.map], [want[k] for k in ("mp", "mr", "mf1", "map50", "map")],
                               rtol=0, atol=1e-12, err_msg=name)


@pytest.fixture(scope="module")
def prg(golden):
    return golden("pr_metric_cases")


def test_fixture_cases_equal_reference(prg):
    for name, nc, se, hw, batches in fixture_cases(prg):
        pm = M.PrMetric(nc, confusion=True)
        _feed(pm, batches, hw, se)
        tp, conf, cls = _records(pm)
        ref, want = R.PrMetricRef(nc, confusion=True), None
        for rows, count, targets, shapes in batches:
            ref.update(rows, count, targets, hw, shapes, se)
        want = ref.compute()
        assert np.array_equal(tp, _ref_tp(ref)), name
        res = pm.compute()
        _assert_same(res, want, name)
        assert np.array_equal(res.matrix, prg[name + "/matrix"]), name
        assert np.allclose(res.pr_metric_result, prg[name + "/result"], rtol=0, atol=1e-12), name
        if name + "/p" in prg:
            for k in ("p", "r", "f1", "ap", "py"):
                np.testing.assert_allclose(getattr(res, k), prg[name + "/" + k], rtol=0, atol=1e-12, err_msg="%s %s" % (name, k))
            assert res.f1_index == int(prg[name + "/f1_index"])


def test_threshold_equality_exact(prg):
    name, nc, se, hw, batches = [c for c in fixture_cases(prg) if c[0] == "threshold_equal"][0]
    pm = M.PrMetric(nc, confusion=True)
    _feed(pm, batches, hw, se)
    tp, _, _ = _records(pm)
    assert np.array_equal(tp, prg[name + "/pb"])
    assert np.array_equal(pm.compute().matrix, prg[name + "/matrix"])


def _random_batch(rs, B, max_det, nc, max_labels, H=640, W=640):
    rows = np.zeros((B, max_det, 6), np.float32)
    count = np.zeros(B, np.int32)
    tg, shapes = [], []
    for b in range(B):
        h0, w0 = [(480, 640), (1080, 1920), (333, 500), (640, 480)][rs.randint(4)]
        r = min(H / h0, W / w0)
        nh, nw = int(round(h0 * r)), int(round(w0 * r))
        shapes.append(((h0, w0), ((nh / h0, nw / w0), ((W - nw) / 2, (H - nh) / 2))))
        nl = rs.randint(0, max_labels + 1)
        wh = rs.uniform(4, 200, (nl, 2))
        xy = rs.uniform(0, 1, (nl, 2)) * ([W, H] - wh)
        lc = rs.randint(0, nc, nl)
        t = np.concatenate([np.full((nl, 1), b), lc[:, None], (xy + wh / 2) / [W, H], wh / [W, H]], 1)
        tg.append(t)
        n = rs.randint(0, max_det + 1) if rs.rand() < 0.9 else 0
        src = rs.randint(0, max(nl, 1), n)
        box = np.concatenate([xy, xy + wh], 1)[src] if nl else rs.uniform(0, 600, (n, 4))
        box = box + rs.normal(0, 6, (n, 4))
        fp = rs.rand(n) < 0.3
        box[fp] = rs.uniform(0, 600, (fp.sum(), 4))
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2] + 1)
        cls = np.where(rs.rand(n) < 0.8, lc[src] if nl else 0, rs.randint(0, nc, n))
        conf = rs.uniform(0.03, 1, n).astype(np.float32)
        if n:
            conf[rs.randint(0, n, max(1, n // 20))] = conf[0]        # some equal confidences: the stable rule decides
        rows[b, :n] = np.concatenate([box, conf[:, None], cls[:, None]], 1)
        count[b] = n
    targets = np.concatenate([tg[b] for b in rs.permutation(B)], 0).astype(np.float32)   # shuffled image order, target order kept
    return rows, count, targets, shapes


@pytest.mark.parametrize("B,max_det", [(1, 300), (7, 1000), (32, 300), (64, 1000)])
def test_random_batches_equal_restatement(B, max_det):
    rs = np.random.RandomState(B * 7 + max_det)
    nc = 12
    batches = [_random_batch(rs, B, max_det, nc, 300 if B <= 7 else 40) for _ in range(2)]
    pm = M.PrMetric(nc, confusion=True)
    ref = R.PrMetricRef(nc, confusion=True)
    for rows, count, targets, shapes in batches:
        pm.update(torch.from_numpy(rows).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(targets).to(DEV), (640, 640), shapes)
        ref.update(rows, count, targets, (640, 640), shapes)
    tp, conf, cls = _records(pm)
    assert np.array_equal(tp, _ref_tp(ref))
    _assert_same(pm.compute(), ref.compute(), "B%d md%d" % (B, max_det))


def _synthetic_stream(pm, images, bs, nc, max_det, labels_per_img, seed):
    """Device-generated batches (NMS-like rows + targets); returns the target classes fed."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    tcls = []
    shapes = [((640, 640), ((1.0, 1.0), (0.0, 0.0)))] * bs
    for i in range(0, images, bs):
        B = min(bs, images - i)
        nl = labels_per_img * B
        lxy = torch.rand(nl, 2, device=DEV, generator=g) * 500
        lwh = torch.rand(nl, 2, device=DEV, generator=g) * 120 + 8
        lcls = torch.randint(0, nc, (nl,), device=DEV, generator=g).float()
        img = torch.arange(B, device=DEV).repeat_interleave(labels_per_img).float()
        targets = torch.cat([img[:, None], lcls[:, None], (lxy + lwh / 2) / 640, lwh / 640], 1)
        src = torch.randint(0, labels_per_img, (B, max_det), device=DEV, generator=g) + torch.arange(B, device=DEV)[:, None] * labels_per_img
        box = torch.cat([lxy, lxy + lwh], 1)[src] + torch.randn(B, max_det, 4, device=DEV, generator=g) * 10
        box[..., 2:] = torch.maximum(box[..., 2:], box[..., :2] + 1)
        cls = torch.where(torch.rand(B, max_det, device=DEV, generator=g) < 0.7, lcls[src], torch.randint(0, nc, (B, max_det), device=DEV, generator=g).float())
        conf = (torch.rand(B, max_det, device=DEV, generator=g) * 0.97 + 0.03).half().float()     # fp16 scores: many equal confidences
        rows = torch.cat([box, conf[..., None], cls[..., None]], 2).contiguous()
        count = torch.full((B,), max_det, dtype=torch.int32, device=DEV)
        pm.update(rows, count, targets, (640, 640), shapes[:B])
        tcls.append(lcls)
    return torch.cat(tcls).cpu().numpy().astype(np.float64)


def _check_curves_against_ap_per_class(pm, tcls):
    tp, conf, cls = _records(pm)
    res = pm.compute()
    p, r, ap, f1, ac, py = R.ap_per_class(tp, conf, cls, tcls)
    k, mp, mr, mf1, map50, map_ = R.summary(p, r, ap, f1)
    for name, got, want in (("p", res.p, p), ("r", res.r, r), ("f1", res.f1, f1), ("ap", res.ap, ap), ("py", res.py, py)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=name)
    assert res.f1_index == k and np.array_equal(res.ap_class, ac)
    np.testing.assert_allclose([res.mp, res.mr, res.mf1, res.map50, res.map], [mp, mr, mf1, map50, map_], rtol=0, atol=1e-12)
    return res


def test_val2017_sized_run():
    pm = M.PrMetric(80)
    tcls = _synthetic_stream(pm, 5000, 32, 80, 300, 7, seed=5)
    res = _check_curves_against_ap_per_class(pm, tcls)
    assert res.seen == 5000 and res.nt.sum() == 35000 and res.ok


def test_single_class_million_records():
    pm = M.PrMetric(1)
    tcls = _synthetic_stream(pm, 3500, 64, 1, 300, 5, seed=6)
    assert int(pm.offs[pm.batches].item()) >= 1_000_000
    _check_curves_against_ap_per_class(pm, tcls)


def test_ap_per_class_surface():
    rs = np.random.RandomState(3)
    n = 5000
    tp = rs.rand(n, 10) < 0.4
    conf = rs.rand(n).astype(np.float32)
    pcls = rs.randint(0, 9, n).astype(np.float32)
    tcls = rs.randint(0, 7, 800).astype(np.float32)
    got = M.metrics.ap_per_class(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pcls).to(DEV),
                                 torch.from_numpy(tcls).to(DEV))
    want = R.ap_per_class(tp, conf, pcls, tcls)[:5]
    for g_, w_ in zip(got[:4], want[:4]):
        np.testing.assert_allclose(g_, w_, rtol=0, atol=1e-12)
    assert np.array_equal(got[4], want[4])


def test_process_batch_and_confusion_surface(prg):
    rs = np.random.RandomState(4)
    rows, count, targets, shapes = _random_batch(rs, 1, 300, 6, 50)
    n = int(count[0])
    det = rows[0, :n]
    lab = targets[:, 1:].copy()
    lab[:, 1:] = R.label_boxes(lab[:, 1:], 640, 640)
    c = M.metrics.process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV))
    assert c.dtype == torch.bool and c.is_cuda
    assert np.array_equal(c.cpu().numpy(), R.process_batch(det, lab))
    cm = M.metrics.ConfusionMatrix(6)
    cm.process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV))
    cm.process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV))
    want = R.confusion_update(R.confusion_update(np.zeros((7, 7)), det, lab, 6), det, lab, 6)
    assert np.array_equal(cm.matrix, want)
    tp, fp = cm.tp_fp()
    assert np.array_equal(tp, want.diagonal()[:-1]) and np.array_equal(fp, (want.sum(1) - want.diagonal())[:-1])


def test_degenerate_results():
    shapes = [((640, 640), ((1.0, 1.0), (0.0, 0.0)))] * 2
    tg = torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2], [1, 2, 0.3, 0.3, 0.1, 0.1]], device=DEV)
    rows = torch.zeros(2, 300, 6, device=DEV)
    pm = M.PrMetric(4)                                      # no detections at all
    pm.update(rows, torch.zeros(2, dtype=torch.int32, device=DEV), tg, (640, 640), shapes)
    res = pm.compute()
    assert res.pr_metric_result == (0.0, 0.0) and not res.ok and res.nt.tolist() == [0, 1, 1, 0] and res.seen == 2
    rows[:, :3] = torch.tensor([[10, 10, 50, 50, 0.9, 1], [100, 100, 150, 150, 0.5, 2], [0, 0, 5, 5, 0.1, 3]], device=DEV)
    pm = M.PrMetric(4, confusion=True)                      # no labels at all
    pm.update(rows, torch.full((2,), 3, dtype=torch.int32, device=DEV), torch.zeros(0, 6, device=DEV), (640, 640), shapes)
    res = pm.compute()
    assert res.pr_metric_result == (0.0, 0.0) and res.nt.sum() == 0 and res.matrix.sum() == 0
    pm = M.PrMetric(4)                                      # labels and detections, nothing correct
    pm.update(rows, torch.full((2,), 3, dtype=torch.int32, device=DEV), tg, (640, 640), shapes)
    assert pm.compute().pr_metric_result == (0.0, 0.0)


def test_device_errors_raise_at_compute():
    shapes = [((640, 640), ((1.0, 1.0), (0.0, 0.0)))]
    rows = torch.zeros(1, 300, 6, device=DEV)
    rows[0, 0] = torch.tensor([10, 10, 50, 50, 0.9, 1], device=DEV)
    cnt = torch.ones(1, dtype=torch.int32, device=DEV)
    pm = M.PrMetric(4)
    pm.update(rows, cnt, torch.tensor([[0, 4, 0.5, 0.5, 0.2, 0.2]], device=DEV), (640, 640), shapes)      # class 4 of nc = 4
    pm.update(rows, cnt, torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2]], device=DEV), (640, 640), shapes)      # a later good batch: no raise
    with pytest.raises(lib.MafError, match="class"):
        pm.compute()
    pm = M.PrMetric(4)
    many = torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2]], device=DEV).repeat(lib.PR_MAX_LABELS + 1, 1)
    pm.update(rows, cnt, many, (640, 640), shapes)
    with pytest.raises(lib.MafError, match="labels"):
        pm.compute()


@pytest.fixture(scope="module")
def model_n():
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", seed=0, cls_bias=-3.0))
    return m.to(DEV).eval()


def _loader(model, seed):
    """Seeded uint8 batches whose targets are jittered copies of some detections of the model itself (so that some are correct)."""
    rs = np.random.RandomState(seed)
    out = []
    for bi, B in enumerate((4, 3)):
        imgs = torch.from_numpy(rs.randint(0, 256, (B, 3, 256, 256)).astype(np.uint8))
        with torch.no_grad():
            model.precision = "fp16"
            pred = model(imgs.to(DEV))[0]
        rows, _, cnt = M.nms_raw(pred, 0.03, 0.65, multi_label=True)
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        tg = []
        for b in range(B):
            for k in rs.permutation(int(cnt[b]))[:6]:
                x1, y1, x2, y2, _, c = rows[b, k]
                j = rs.normal(0, 2, 4)
                x1, y1, x2, y2 = x1 + j[0], y1 + j[1], max(x2 + j[2], x1 + j[0] + 1), max(y2 + j[3], y1 + j[1] + 1)
                tg.append([b, c, (x1 + x2) / 512, (y1 + y2) / 512, (x2 - x1) / 256, (y2 - y1) / 256])
        shapes = [((480, 640), ((0.4, 0.4), (0.0, 32.0))), ((256, 256), ((1.0, 1.0), (0.0, 0.0))), ((333, 500), ((0.512, 0.512), (0.0, 42.75))),
                  ((640, 480), ((0.4, 0.4), (32.0, 0.0)))][:B]
        paths = ["/x/%012d.jpg" % (100 * bi + b) for b in range(B)]
        out.append((imgs, torch.tensor(tg, dtype=torch.float32).reshape(-1, 6), paths, shapes))
    return out


def test_eval_loop_pr_metric_end_to_end(model_n, monkeypatch):
    loader = _loader(model_n, 9)
    base = EL.EvalLoop(model_n, half=True, ids=list(range(80)))
    rows_plain = base.predict_model(loader)
    assert base.pr_metric_result is None and base.pr_metric is None
    seen_rows = []
    real = EL._nms.nms_raw

    def capture(*a, **k):
        r = real(*a, **k)
        seen_rows.append((r[0].cpu().numpy(), r[2].cpu().numpy()))
        return r

    monkeypatch.setattr(EL._nms, "nms_raw", capture)
    loop = EL.EvalLoop(model_n, half=True, ids=list(range(80)), do_pr_metric=True, plot_confusion_matrix=True)
    rows_pr = loop.predict_model(loader)
    assert rows_pr == rows_plain
    ref = R.PrMetricRef(80, confusion=True)
    for (rows, cnt), (imgs, targets, paths, shapes) in zip(seen_rows, loader):
        ref.update(rows, cnt, targets.numpy(), imgs.shape[2:], shapes)
    want = ref.compute()
    assert "p" in want, "the synthetic targets should make some detections correct"
    _assert_same(loop.pr_metric, want, "eval_loop")
    assert loop.pr_metric_result == loop.pr_metric.pr_metric_result


def test_update_does_not_sync_and_compute_syncs_once():
    rs = np.random.RandomState(12)
    batches = [_random_batch(rs, 8, 300, 5, 20) for _ in range(3)]
    dev_batches = [(torch.from_numpy(r).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(t).to(DEV), s) for r, c, t, s in batches]
    warm = M.PrMetric(5, confusion=True)                    # library loaded, pinned pool primed
    warm.update(*dev_batches[0][:3], (640, 640), dev_batches[0][3])
    warm.compute()
    torch.cuda.synchronize()
    pm = M.PrMetric(5, confusion=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for r, c, t, s in dev_batches:
            pm.update(r, c, t, (640, 640), s)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            pm.compute()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    syncs = [x for x in w if "synchroniz" in str(x.message)]
    assert len(syncs) == 1, [str(x.message) for x in syncs]
