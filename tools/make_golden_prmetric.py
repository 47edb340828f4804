#!/usr/bin/env python3
"""Golden vectors for the in-process precision / recall / mAP (`do_pr_metric`): the reference's OWN Evaler.predict_model statistics block
(yolov6/core/evaler.py:143-151, 182-238, 240-271) with its process_batch, ConfusionMatrix and ap_per_class (yolov6/utils/metrics.py), run
here in the build container on seeded synthetic detections.

    python tools/make_golden_prmetric.py    ->  tests/golden/pr_metric_cases.npz

predict_model runs as it is: the model is a stub and the module's non_max_suppression is replaced by one that hands back this script's
detections, so everything after the NMS — the deep copy, scale_coords (bound to an Evaler built without its data loader), xywh2xyxy,
process_batch, ConfusionMatrix.process_batch, ap_per_class, the F1 index and the summary — is the reference's code.  process_batch's
results, ap_per_class's inputs and outputs, and the precision curve ap_per_class hands to plot_pr_curve (py) are captured by wrappers.

The data have no IoU ties within an image and no confidence ties within a case, and the F1 maximum is separated from its runner-up by more
than 1e-9, so the reference's unstable orderings cannot change the result: the script asserts all three.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_DET = 300
F32 = np.float32


def _shape(h0, w0, H, W):
    r = min(H / h0, W / w0)
    nh, nw = int(round(h0 * r)), int(round(w0 * r))
    return ((h0, w0), ((nh / h0, nw / w0), ((W - nw) / 2, (H - nh) / 2)))


def _image(rs, b, H, W, nl, nc, absent=(), mode="mix"):
    """One image: (targets [nl, 5] cls + normalised xywh, detections [nd, 6] letterboxed xyxy + conf + cls)."""
    lab_px, lab_cls, dets = [], [], []
    for _ in range(nl):
        w, h = rs.uniform(12, W / 3), rs.uniform(12, H / 3)
        x1, y1 = rs.uniform(0, W - w), rs.uniform(0, H - h)
        c = int(rs.randint(0, nc))
        while c in absent:
            c = int(rs.randint(0, nc))
        lab_px.append((x1, y1, x1 + w, y1 + h))
        lab_cls.append(c)
    lab_px = np.asarray(lab_px, np.float64).reshape(-1, 4)
    for l in range(nl):
        x1, y1, x2, y2 = lab_px[l]
        w, h = x2 - x1, y2 - y1
        for _ in range(rs.choice([0, 1, 1, 1, 2, 3]) if mode != "nothing" else 1):
            j = rs.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h]) if mode != "nothing" else np.array([w * 0.9, 0, w * 0.9, 0])
            c = lab_cls[l] if rs.rand() < 0.8 else int(rs.randint(0, nc))
            if mode == "nothing":                                               # shifted off its label and of another class
                c = (lab_cls[l] + 1) % nc
            dets.append((x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3], c))
    for _ in range(rs.randint(0, 6) if mode != "nothing" else 0):              # false positives, some of an absent class
        w, h = rs.uniform(8, W / 4), rs.uniform(8, H / 4)
        x1, y1 = rs.uniform(0, W - w), rs.uniform(0, H - h)
        c = int(absent[0]) if (absent and rs.rand() < 0.5) else int(rs.randint(0, nc))
        dets.append((x1, y1, x1 + w, y1 + h, c))
    if nl >= 2 and mode == "mix":                                               # one detection over two labels
        a, bb = lab_px[0], lab_px[1]
        dets.append(((a[0] + bb[0]) / 2, (a[1] + bb[1]) / 2, (a[2] + bb[2]) / 2, (a[3] + bb[3]) / 2, lab_cls[0]))
    dets = dets[:MAX_DET]
    d = np.zeros((len(dets), 6), F32)
    if len(dets):
        arr = np.asarray(dets, np.float64)
        d[:, :4] = np.clip(arr[:, :4], -4, max(H, W) + 4)
        d[:, 5] = arr[:, 4]
    t = np.zeros((nl, 5), F32)
    if nl:
        xy = (lab_px[:, :2] + lab_px[:, 2:]) / 2
        wh = lab_px[:, 2:] - lab_px[:, :2]
        t[:, 0] = lab_cls
        t[:, 1:] = np.concatenate([xy / [W, H], wh / [W, H]], 1)
    return t, d


def _threshold_images(iouv):
    """Images of a 640 x 640 letterbox with gain 1 and no padding: one label [0, 0, 100, 100] of class 0 and one detection [0, 0, 100, h]
    whose fp32 IoU equals a threshold exactly (or is the nearest reachable fp32 IoU below / above it).  Each pair sits in its own image."""
    from pr_metric_ref import box_iou
    lab = np.array([[0, 0, 100, 100]], F32)
    out = []
    targets = list(iouv.tolist()) + [F32(0.45)]
    for t in targets:
        t = F32(t)
        iou = lambda h: box_iou(lab, np.array([[0, 0, 100, h]], F32))[0, 0]
        h = F32(float(t) * 100.0)
        for _ in range(64):                                                    # exactly t
            if iou(h) == t:
                break
            h = np.nextafter(h, F32(200) if iou(h) < t else F32(0))
        assert iou(h) == t, t
        lo = hi = h
        while iou(lo) >= t:                                                    # the largest reachable IoU below t
            lo = np.nextafter(lo, F32(0))
        while iou(hi) <= t:                                                    # the smallest reachable IoU above t
            hi = np.nextafter(hi, F32(200))
        out += [h, lo, hi]
    return out


def cases(iouv):
    """[(name, nc, scale_exact, H, W, batches)], batches = [(targets [N, 6], detections list, shapes)]."""
    rs = np.random.RandomState(20261015)
    out = []
    shp = [(480, 640), (427, 640), (1080, 1920), (333, 500), (640, 480), (500, 375)]

    def batch(B, H, W, nc, nl_fn, **kw):
        tg, dets, shapes = [], [], []
        order = rs.permutation(B)                                               # targets in shuffled image order, target order kept
        per = {}
        for b in range(B):
            h0, w0 = shp[rs.randint(len(shp))]
            shapes.append(_shape(h0, w0, H, W))
            t, d = _image(rs, b, H, W, nl_fn(b), nc, **kw)
            per[b] = t
            dets.append(d)
        for b in order:
            t = per[b]
            tg.append(np.concatenate([np.full((len(t), 1), b, F32), t], 1))
        return np.concatenate(tg, 0).reshape(-1, 6), dets, shapes

    out.append(("mixed", 80, False, 640, 640, [batch(8, 640, 640, 80, lambda b: rs.randint(1, 13)) for _ in range(2)]))
    out.append(("mixed_exact_rect", 20, True, 384, 640, [batch(6, 384, 640, 20, lambda b: rs.randint(1, 9)) for _ in range(2)]))
    out.append(("crowded", 5, False, 640, 640, [batch(2, 640, 640, 5, lambda b: 110 + 20 * b)]))
    # images with no predictions, no labels, or neither
    tg, dets, shapes = batch(6, 640, 640, 10, lambda b: [0, 5, 3, 0, 7, 2][b])
    dets[1] = dets[1][:0]
    dets[3] = dets[3][:0]
    dets[2] = dets[2][:0]
    out.append(("empty_images", 10, False, 640, 640, [(tg, dets, shapes)]))
    out.append(("absent_classes", 12, False, 640, 640, [batch(5, 640, 640, 12, lambda b: rs.randint(2, 9), absent=(3, 7))]))
    out.append(("nothing_correct", 8, False, 640, 640, [batch(4, 640, 640, 8, lambda b: rs.randint(1, 5), mode="nothing")]))
    # threshold equality: one label + one detection per image, no rescale
    hs = _threshold_images(iouv)
    tg, dets, shapes = [], [], []
    for b, h in enumerate(hs):
        tg.append([b, 0, 50 / 640, 50 / 640, 100 / 640, 100 / 640])
        dets.append(np.array([[0, 0, 100, h, 0.3 + 0.6 * b / len(hs), 0]], F32))
        shapes.append(((640, 640), ((1.0, 1.0), (0.0, 0.0))))
    out.append(("threshold_equal", 2, False, 640, 640, [(np.asarray(tg, F32), dets, shapes)]))
    return out


def _assign_conf(rs, dets):
    n = sum(len(d) for d in dets)
    conf = (rs.permutation(n) + rs.uniform(0.05, 0.95, n)) / n * 0.97 + 0.03
    i = 0
    for d in dets:
        d[:, 4] = conf[i:i + len(d)]
        i += len(d)


def run_reference(Evaler, metrics, name, nc, scale_exact, H, W, batches):
    import yolov6.core.evaler as evaler_mod
    captured = {"pb": [], "ap_in": None, "ap_out": None, "py": None, "cm": None}
    real_pb, real_ap, real_cm = metrics.process_batch, metrics.ap_per_class, metrics.ConfusionMatrix

    def pb(detections, labels, iouv):
        c = real_pb(detections, labels, iouv)
        iou = metrics.general.box_iou(labels[:, 1:], detections[:, :4]).numpy()
        for row in iou:                                                       # no IoU ties within an image (per detection / per label)
            nz = row[row > 0]
            assert len(np.unique(nz)) == len(nz), "%s: IoU tie" % name
        for col in iou.T:
            nz = col[col > 0]
            assert len(np.unique(nz)) == len(nz), "%s: IoU tie" % name
        captured["pb"].append(c.numpy())
        return c

    def ap(*a, **k):
        captured["ap_in"] = [np.asarray(x) for x in a]
        res = real_ap(*a, **k)
        captured["ap_out"] = res
        return res

    class CM(real_cm):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            captured["cm"] = self

        def plot(self, *a, **k):
            pass

    def plot_pr(px, py, ap_, *a, **k):
        captured["py"] = np.stack(py, 0) if len(py) else np.zeros((0, 1000))

    metrics.process_batch, metrics.ap_per_class, metrics.ConfusionMatrix = pb, ap, CM
    metrics.plot_pr_curve, metrics.plot_mc_curve = plot_pr, lambda *a, **k: None
    queue = []
    evaler_mod.non_max_suppression = lambda outputs, *a, **k: queue.pop(0)

    class StubModel:
        def __init__(self):
            self.nc, self.names = nc, ["c%d" % i for i in range(nc)]

        def __call__(self, imgs):
            return imgs, None

    ev = Evaler.__new__(Evaler)
    ev.device, ev.half, ev.conf_thres, ev.iou_thres = torch.device("cpu"), False, 0.03, 0.65
    ev.do_pr_metric, ev.plot_confusion_matrix, ev.plot_curve, ev.verbose = True, True, True, False
    ev.scale_exact, ev.is_coco, ev.save_dir, ev.ids = scale_exact, True, "/nonexistent", list(range(nc))
    loader, img_no = [], 1
    for targets, dets, shapes in batches:
        B = len(dets)
        queue.append([torch.from_numpy(d.copy()) for d in dets])
        paths = ["/x/%012d.jpg" % (img_no + b) for b in range(B)]
        img_no += B
        loader.append((torch.zeros(B, 3, H, W, dtype=torch.uint8), torch.from_numpy(targets), paths, shapes))
    ev.predict_model(StubModel(), loader, "val")
    metrics.process_batch, metrics.ap_per_class, metrics.ConfusionMatrix = real_pb, real_ap, real_cm
    return captured, ev.pr_metric_result


def main():
    import make_golden_post
    Evaler = make_golden_post.load_evaler()
    import yolov6.utils.metrics as metrics
    iouv = torch.linspace(0.5, 0.95, 10).numpy()
    rs = np.random.RandomState(7)
    blob = {"iouv": iouv}
    names = []
    for name, nc, scale_exact, H, W, batches in cases(iouv):
        dets_all = [d for _, dets, _ in batches for d in dets]
        if name != "threshold_equal":
            _assign_conf(rs, dets_all)
        confs = np.concatenate([d[:, 4] for d in dets_all])
        assert len(np.unique(confs)) == len(confs), "%s: confidence tie" % name
        cap, res = run_reference(Evaler, metrics, name, nc, scale_exact, H, W, batches)
        pre = "%s/" % name
        names.append(name)
        blob[pre + "meta"] = np.array([nc, int(scale_exact), H, W, len(batches)], np.int64)
        for bi, (targets, dets, shapes) in enumerate(batches):
            B = len(dets)
            cnt = np.array([len(d) for d in dets], np.int32)
            rows = np.zeros((B, max(1, int(cnt.max())), 6), F32)              # nms_raw's layout, trimmed to the longest image
            for b, d in enumerate(dets):
                rows[b, :len(d)] = d
            blob[pre + "rows%d" % bi] = rows
            blob[pre + "count%d" % bi] = cnt
            blob[pre + "targets%d" % bi] = targets
            blob[pre + "shapes%d" % bi] = np.array([[s[0][0], s[0][1], s[1][0][0], s[1][0][1], s[1][1][0], s[1][1][1]] for s in shapes], np.float64)
        blob[pre + "pb"] = np.concatenate(cap["pb"], 0) if cap["pb"] else np.zeros((0, 10), bool)
        blob[pre + "matrix"] = cap["cm"].matrix
        blob[pre + "result"] = np.array(res, np.float64)
        if cap["ap_out"] is not None:
            tp, conf, pcls, tcls = cap["ap_in"]
            p, r, ap, f1, ap_class = cap["ap_out"]
            m = f1.mean(0)
            k = len(m) - m[::-1].argmax() - 1
            rest = m[m != m[k]]
            assert rest.size == 0 or m[k] - rest.max() > 1e-9, "%s: F1 maximum not separated" % name
            has_pred = np.array([(pcls == c).sum() > 0 for c in ap_class])
            py = np.zeros((len(ap_class), 1000))
            py[has_pred] = cap["py"]
            blob.update({pre + "tp": tp, pre + "conf": conf, pre + "pred_cls": pcls, pre + "target_cls": tcls, pre + "p": p, pre + "r": r,
                         pre + "ap": ap, pre + "f1": f1, pre + "ap_class": ap_class, pre + "py": py, pre + "f1_index": np.int64(k),
                         pre + "nt": np.bincount(tcls.astype(np.int64), minlength=nc),
                         pre + "summary": np.array([p[:, k].mean(), r[:, k].mean(), m[k], ap[:, 0].mean(), ap.mean(1).mean()])})
        print("%-18s nc %3d  images %3d  rows %5d  result %s" % (name, nc, sum(len(d) for _, d, _ in batches), len(confs), tuple(res)))
    blob["cases"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pr_metric_cases.npz"), **blob)


if __name__ == "__main__":
    main()
