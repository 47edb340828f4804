"""Host tests of the COCOeval restatement (tests/cocoeval_ref.py): hand cases with known answers, the pycocotools cross-check where it is
installed, and the errors maf_yolo_amd.cocoeval raises without a HIP device."""
import numpy as np
import pytest
import torch

import cocoeval_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import cocoeval as CE

EPS = 2.220446049250313e-16
PERFECT = 1.0 / (1.0 + EPS)


def anno(gts, images=(1,), cats=(1,)):
    """gts: (image_id, category_id, bbox, extra dict) -> instances dict; ids 1.. in list order unless extra gives one."""
    anns = []
    for j, (im, c, bb, *extra) in enumerate(gts):
        a = {"id": j + 1, "image_id": im, "category_id": c, "bbox": list(bb), "area": bb[2] * bb[3], "iscrowd": 0}
        if extra:
            a.update(extra[0])
        anns.append(a)
    return {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats], "annotations": anns}


def det(im, c, bb, s):
    return {"image_id": im, "category_id": c, "bbox": list(bb), "score": s}


def test_perfect_detection():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10])]), [det(1, 1, [0, 0, 10, 10], .9)])
    p = ev.eval["precision"]
    assert np.all(p[:, :, 0, 0, 2] == PERFECT) and PERFECT == 0.9999999999999998
    assert ev.stats[0] == PERFECT and "%.3f" % ev.stats[0] == "1.000"
    assert ev.stats[8] == 1.0 and ev.stats[6] == 1.0
    assert ev.stats[3] == ev.stats[0] and ev.stats[4] == -1 and ev.stats[5] == -1


def test_higher_scored_false_positive():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10])]), [det(1, 1, [50, 50, 10, 10], .95), det(1, 1, [0, 0, 10, 10], .9)])
    assert ev.stats[0] == pytest.approx(0.5, abs=1e-12)
    assert ev.stats[6] == 0.0 and ev.stats[8] == 1.0


def test_iou_exactly_half():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10])]), [det(1, 1, [0, 0, 10, 5], .9)])
    p = ev.eval["precision"][:, :, 0, 0, 2]
    assert np.all(p[0] == PERFECT) and np.all(p[5] == 0.0) and ev.stats[2] == 0.0
    assert ev.stats[0] == pytest.approx(0.1, abs=1e-12)


@pytest.mark.parametrize("a_first", [True, False])
def test_equal_iou_goes_to_later_gt(a_first):
    A, B = [0, 0, 10, 10], [10, 0, 10, 10]
    gts = [(1, 1, A), (1, 1, B)] if a_first else [(1, 1, B), (1, 1, A)]
    ev = R.run(anno(gts), [det(1, 1, [0, 0, 20, 10], .9), det(1, 1, [0, 0, 10, 10], .8)])
    if a_first:     # d1 takes B (the later gt), d2 takes A
        assert ev.stats[1] == 1.0
    else:           # d1 takes A, d2 has only A at IoU >= .5 and it is taken: a false positive
        assert ev.stats[1] < 0.99


def test_detection_in_crowd_is_ignored():
    gts = [(1, 1, [0, 0, 10, 10]), (1, 1, [100, 100, 50, 50], {"iscrowd": 1})]
    with_crowd = R.run(anno(gts), [det(1, 1, [110, 110, 10, 10], .95), det(1, 1, [0, 0, 10, 10], .9)])
    assert np.all(with_crowd.eval["precision"][0, :, 0, 0, 2] == PERFECT)


def test_area_1024_is_small_and_medium():
    ev = R.run(anno([(1, 1, [0, 0, 32, 32])]), [det(1, 1, [0, 0, 32, 32], .9)])
    assert ev.stats[3] == PERFECT and ev.stats[4] == PERFECT and ev.stats[5] == -1


def test_annotation_id_zero_is_a_false_positive():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10], {"id": 0})]), [det(1, 1, [0, 0, 10, 10], .9)])
    assert ev.stats[0] == 0.0 and ev.stats[8] == 0.0


def test_category_without_gts_is_minus_one_and_excluded():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10])], cats=(1, 7)), [det(1, 1, [0, 0, 10, 10], .9), det(1, 7, [0, 0, 10, 10], .8)])
    assert np.all(ev.eval["precision"][:, :, 1] == -1) and np.all(ev.eval["recall"][:, 1] == -1)
    assert ev.stats[0] == PERFECT


def test_ar1_differs_from_ar10():
    ev = R.run(anno([(1, 1, [0, 0, 10, 10]), (1, 1, [50, 50, 10, 10])]), [det(1, 1, [0, 0, 10, 10], .9), det(1, 1, [50, 50, 10, 10], .8)])
    assert ev.stats[6] == 0.5 and ev.stats[7] == 1.0


def test_string_image_ids():
    gts = [("b", 1, [0, 0, 10, 10]), ("a", 1, [0, 0, 10, 10])]
    ev = R.run(anno(gts, images=("b", "a")), [det("a", 1, [0, 0, 10, 10], .9)])
    assert ev.params.imgIds == ["a", "b"]
    assert ev.stats[8] == 0.5


def test_foreign_image_id_asserts():
    with pytest.raises(AssertionError):
        R.run(anno([(1, 1, [0, 0, 10, 10])]), [det(2, 1, [0, 0, 10, 10], .9)])


def _random_set(seed, n_img=12, n_cat=4):
    rs = np.random.RandomState(seed)
    cats = [3, 9, 17, 40][:n_cat]
    gts, dts = [], []
    for im in range(n_img):
        for _ in range(rs.randint(0, 6)):
            bb = [float(v) for v in np.round(rs.uniform(0, 200, 4) * [1, 1, .5, .5], 2)]
            gts.append((im, int(rs.choice(cats)), bb, {"iscrowd": int(rs.rand() < .1)}))
        for _ in range(rs.randint(0, 12)):
            bb = [float(v) for v in np.round(rs.uniform(0, 200, 4) * [1, 1, .5, .5], 3)]
            dts.append(det(im, int(rs.choice(cats)), bb, float(np.round(rs.rand(), 5))))
    return anno(gts, images=range(n_img), cats=cats), dts


def test_cross_check_against_pycocotools(capsys):
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    for seed in range(3):
        gt, dts = _random_set(seed)
        want = R.run(gt, dts)
        coco = COCO()
        coco.dataset = gt
        coco.createIndex()
        ev = COCOeval(coco, coco.loadRes(dts), "bbox")
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(ev.eval[k], want.eval[k]), k
        assert np.array_equal(ev.stats, want.stats)


def test_summarize_prints_pycocotools_lines(capsys):
    ev = R.run(anno([(1, 1, [0, 0, 10, 10])]), [det(1, 1, [0, 0, 10, 10], .9)])
    p = CE.Params.__new__(CE.Params)
    for k, v in CE._default_params().items():
        setattr(p, k, v)
    stats = CE.summarize(ev.eval, p)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 12
    assert out[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert out[4] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000"
    assert out[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000"
    assert np.array_equal(stats, ev.stats)


def test_cpu_device_raises():
    with pytest.raises(M.MafError):
        M.CocoGt(anno([(1, 1, [0, 0, 10, 10])]), device="cpu")


def test_cpu_tensors_raise_in_update():
    ev = CE.CocoEval.__new__(CE.CocoEval)
    ev.gt = None
    with pytest.raises(M.MafError):
        CE.CocoEval.update(ev, torch.zeros(4, 7), torch.zeros(1, dtype=torch.int32), [1])


def test_coco_eval_takes_a_coco_gt():
    with pytest.raises(M.MafError):
        M.CocoEval(anno([(1, 1, [0, 0, 10, 10])]))
