"""CPU tests of the in-process precision / recall / mAP (maf-yolo_amd/metrics.py, csrc/pr_metric.hip): the NumPy restatement
(tests/pr_metric_ref.py) against what the reference's own Evaler.predict_model statistics block computed (tests/golden/pr_metric_cases.npz,
tools/make_golden_prmetric.py), the two tie rules on hand-made cases, and the host-side surface: CPU tensors raise, the ops are declared."""
import numpy as np
import pytest
import torch

import pr_metric_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import lib


def fixture_cases(g):
    """-> [(name, nc, scale_exact, (H, W), [(rows, count, targets, shapes)])] from the fixture."""
    out = []
    for name in g["cases"]:
        nc, se, H, W, nb = (int(v) for v in g[name + "/meta"])
        batches = []
        for i in range(nb):
            sh = g["%s/shapes%d" % (name, i)]
            shapes = [((int(s[0]), int(s[1])), ((float(s[2]), float(s[3])), (float(s[4]), float(s[5])))) for s in sh]
            batches.append((g["%s/rows%d" % (name, i)], g["%s/count%d" % (name, i)], g["%s/targets%d" % (name, i)], shapes))
        out.append((str(name), nc, bool(se), (H, W), batches))
    return out


def run_ref(nc, se, hw, batches, confusion=True):
    ref = R.PrMetricRef(nc, confusion=confusion)
    for rows, count, targets, shapes in batches:
        ref.update(rows, count, targets, hw, shapes, scale_exact=se)
    return ref, ref.compute()


@pytest.fixture(scope="module")
def prg(golden):
    return golden("pr_metric_cases")


def test_fixture_covers_the_issue_cases(prg):
    names = set(str(n) for n in prg["cases"])
    assert {"mixed", "crowded", "empty_images", "absent_classes", "nothing_correct", "threshold_equal"} <= names
    assert np.array_equal(prg["iouv"], torch.linspace(0.5, 0.95, 10).numpy())
    assert prg["crowded/targets0"].shape[0] >= 200
    assert tuple(prg["nothing_correct/result"]) == (0.0, 0.0)


def test_restatement_equals_reference(prg):
    for name, nc, se, hw, batches in fixture_cases(prg):
        ref, res = run_ref(nc, se, hw, batches)
        pb = np.concatenate(ref.correct, 0) if ref.correct else np.zeros((0, 10), bool)
        assert np.array_equal(pb, prg[name + "/pb"]), name
        assert np.array_equal(res["matrix"], prg[name + "/matrix"]), name
        assert res["seen"] == sum(len(b[1]) for b in batches)
        assert (res["map50"], res["map"]) == tuple(prg[name + "/result"]) or np.allclose((res["map50"], res["map"]), prg[name + "/result"],
                                                                                          rtol=0, atol=1e-12), name
        if name + "/p" not in prg:
            assert "p" not in res, name
            continue
        for k in ("p", "r", "f1", "ap", "py"):
            np.testing.assert_allclose(res[k], prg[name + "/" + k], rtol=0, atol=1e-12, err_msg="%s %s" % (name, k))
        assert res["f1_index"] == int(prg[name + "/f1_index"]), name
        assert np.array_equal(res["nt"], prg[name + "/nt"]), name
        assert np.array_equal(res["ap_class"], prg[name + "/ap_class"]), name
        np.testing.assert_allclose([res["mp"], res["mr"], res["mf1"], res["map50"], res["map"]], prg[name + "/summary"], rtol=0, atol=1e-12)


def test_restatement_ap_per_class_equals_reference_inputs(prg):
    # ap_per_class alone, fed the very stats the reference fed its own
    for name in prg["cases"]:
        name = str(name)
        if name + "/tp" not in prg:
            continue
        p, r, ap, f1, ap_class, py = R.ap_per_class(prg[name + "/tp"], prg[name + "/conf"], prg[name + "/pred_cls"], prg[name + "/target_cls"])
        for k, v in (("p", p), ("r", r), ("ap", ap), ("f1", f1), ("py", py)):
            np.testing.assert_allclose(v, prg[name + "/" + k], rtol=0, atol=1e-12, err_msg="%s %s" % (name, k))
        assert np.array_equal(ap_class, prg[name + "/ap_class"])


def test_threshold_equality_pairs(prg):
    # IoU == iouv[t] exactly is correct at t (>=); the nearest IoU below is not; the confusion matrix's iou > 0.45 rejects fp32(0.45)
    iouv = prg["iouv"]
    pb = prg["threshold_equal/pb"]
    for t in range(10):
        eq, lo, hi = pb[3 * t], pb[3 * t + 1], pb[3 * t + 2]
        assert eq[t] and hi[t] and not lo[t], t
        assert eq[:t + 1].all() and not eq[t + 1:].any()
    lab = np.array([[0, 0, 0, 100, 100]], np.float32)
    rows = prg["threshold_equal/rows0"]
    eq45, lo45, hi45 = rows[30, 0], rows[31, 0], rows[32, 0]
    assert R.box_iou(lab[:, 1:], eq45[None, :4])[0, 0] == np.float32(0.45)
    assert iouv.dtype == np.float32
    for det, want in ((eq45, 0), (lo45, 0), (hi45, 1)):
        m = R.confusion_update(np.zeros((3, 3)), det[None], lab, 2)
        assert m[0, 0] == want


def test_tie_rule_iou_lower_label_wins():
    # one detection with the same IoU to labels 0 and 1 (mirror images around it); a second detection only overlaps label 1
    labels = np.array([[0, 0, 0, 10, 10], [0, 10, 0, 20, 10]], np.float32)
    det = np.array([[5, 0, 15, 10, 0.9, 0], [12, 0, 20, 10, 0.8, 0]], np.float32)
    iou = R.box_iou(labels[:, 1:], det[:, :4])
    assert iou[0, 0] == iou[1, 0]
    c = R.process_batch(det, labels, np.array([0.3], np.float32))
    assert c[:, 0].tolist() == [True, True]                 # det 0 took label 0 (lower index), so det 1 keeps label 1
    labels_swapped = labels[::-1].copy()
    c2 = R.process_batch(det, labels_swapped, np.array([0.3], np.float32))
    assert c2[:, 0].tolist() == [True, False]               # now det 0 takes label index 0 = the right box, which det 1 also wanted


def test_tie_rule_confusion_lower_detection_wins():
    labels = np.array([[1, 10, 0, 20, 10]], np.float32)
    det = np.array([[5, 0, 15, 10, 0.9, 2], [15, 0, 25, 10, 0.8, 3]], np.float32)    # equal IoU (1/3) with the label from both sides
    assert R.box_iou(labels[:, 1:], det[:2, :4])[0, 0] == R.box_iou(labels[:, 1:], det[1:, :4])[0, 0]
    m = R.confusion_update(np.zeros((5, 5)), det, labels, 4, iou_thres=0.3)
    assert m[2, 1] == 1 and m[3, 1] == 0                    # the lower detection index is the match
    assert m[3, 4] == 1                                     # the other is an unmatched detection of an image with a match


def test_tie_rule_confidence_stable():
    # equal confidences keep input order (image order, then NMS row order)
    tp = np.array([[True], [False], [True]])
    conf = np.array([0.5, 0.5, 0.4], np.float32)
    p, r, ap, f1, ac, py = R.ap_per_class(tp, conf, np.zeros(3), np.zeros(2))
    p2, r2, ap2, f12, ac2, py2 = R.ap_per_class(tp[[1, 0, 2]], conf[[1, 0, 2]], np.zeros(3), np.zeros(2))
    assert ap[0, 0] != ap2[0, 0]                           # order matters, so the stable rule is what pins it
    assert ap[0, 0] > ap2[0, 0]


def test_metrics_raise_on_cpu_tensors():
    d = torch.zeros(3, 6)
    lab = torch.zeros(2, 5)
    with pytest.raises(lib.MafError):
        M.metrics.process_batch(d, lab)
    with pytest.raises(lib.MafError):
        M.metrics.ConfusionMatrix(4).process_batch(d, lab)
    with pytest.raises(lib.MafError):
        M.metrics.ap_per_class(torch.zeros(3, 10, dtype=torch.bool), torch.zeros(3), torch.zeros(3), torch.zeros(2))
    pm = M.PrMetric(80)
    with pytest.raises(lib.MafError):
        pm.update(torch.zeros(2, 300, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(0, 6), (640, 640), [((640, 640), ((1, 1), (0, 0)))] * 2)
    with pytest.raises(lib.MafError):
        M.metrics.ap_per_class(torch.zeros(3, 10, dtype=torch.bool), torch.zeros(3), torch.zeros(3), torch.zeros(2), plot=True)


def test_prmetric_bounds_and_empty_compute():
    with pytest.raises(lib.MafError):
        M.PrMetric(0)
    with pytest.raises(lib.MafError):
        M.PrMetric(lib.PR_MAX_CLASSES + 1)
    with pytest.raises(lib.MafError):
        M.PrMetric(80, iouv=torch.linspace(0.1, 0.9, 17))
    res = M.PrMetric(5, confusion=True).compute()          # nothing fed: nothing touches the device
    assert res.seen == 0 and res.pr_metric_result == (0.0, 0.0) and res.matrix.shape == (6, 6) and not res.ok


def test_torch_ops_declare_pr_metric():
    from maf_yolo_amd import torch_ops
    assert "pr_match" in torch_ops.OPS and "pr_curves" in torch_ops.OPS


def test_capi_declares_pr_metric():
    assert {"maf_pr_match", "maf_pr_curves", "maf_pr_workspace_bytes", "maf_pr_state_ints", "maf_pr_out_doubles"} <= set(lib.EXPORTS)
    hdr = open(lib.__file__.replace("maf-yolo_amd/lib.py", "include/mafyolo_hip.h")).read()
    for s in ("maf_pr_match", "maf_pr_curves", "maf_pr_workspace_bytes", "MAF_PR_MAX_DET 1024", "MAF_PR_MAX_LABELS 1024"):
        assert s in hdr
