"""GPU tests of the COCO bbox mAP (maf-yolo_amd/cocoeval.py over csrc/cocoeval.hip) against the NumPy restatement of pycocotools' COCOeval
(tests/cocoeval_ref.py): precision, recall, scores and stats exactly equal, -1 included; update() and load_res() of the same rows agree;
EvalLoop(do_coco_metric=True) end to end; the host-sync contract of update(); the errors."""
import importlib
import warnings

import numpy as np
import pytest
import torch

import cocoeval_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import lib
from maf_yolo_amd import post as P
from oracle import maf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EL = importlib.import_module("maf_yolo_amd.eval_loop")


def synth_set(seed, n_img=240, n_cat=30, str_ids=False):
    """A seeded instances dict and detection rows that hit the corner cases: crowd gts, areas on both borders (1024, 9216), shuffled and
    sparse annotation ids with one 0, cells with more than 100 detections, exact score ties, images without gts, unknown categories,
    IoUs exactly on thresholds (.5, .75), zero-width boxes.  Detections: (image id, category id, x, y, w, h, score) as fp32-representable
    values (the device path starts from fp32 rows)."""
    rs = np.random.RandomState(seed)
    cats = sorted(rs.choice(np.arange(1, 200), n_cat, replace=False).tolist())
    imgs = [("im%04d" % i) if str_ids else int(1000 + 7 * i) for i in range(n_img)]
    anns, dets = [], []
    for ii, im in enumerate(imgs):
        if ii % 11 == 5:                                     # an image without gts
            ng = 0
        else:
            ng = rs.randint(0, 9)
        for _ in range(ng):
            c = int(rs.choice(cats[:20]))
            x, y = float(rs.randint(0, 500)), float(rs.randint(0, 400))
            w, h = float(rs.choice([2, 8, 16, 32, 64, 96, 150])), float(rs.choice([4, 16, 32, 48, 96, 200]))
            area = w * h
            r = rs.rand()
            if r < .05:
                area = 1024.0
            elif r < .1:
                area = 9216.0
            crowd = int(rs.rand() < .08)
            anns.append({"image_id": im, "category_id": c, "bbox": [x, y, w, h], "area": area, "iscrowd": crowd})
            # detections around this gt: exact, IoU exactly .5 (half width), exactly .75, jittered
            for kind in rs.choice(4, rs.randint(0, 4)):
                if kind == 0:
                    bb = [x, y, w, h]
                elif kind == 1:
                    bb = [x, y, w / 2, h]
                elif kind == 2:
                    bb = [x, y, w * .75, h]
                else:
                    bb = [x + rs.randint(-4, 5), y + rs.randint(-4, 5), max(0.0, w + rs.randint(-6, 7)), max(0.0, h + rs.randint(-6, 7))]
                dets.append((im, c, *bb, rs.randint(1, 100000) / 100000.0))
        for _ in range(rs.randint(0, 25)):                   # background detections, some of unknown categories, some zero-width
            c = int(rs.choice(cats)) if rs.rand() > .05 else 1000 + rs.randint(0, 5)
            w = 0.0 if rs.rand() < .03 else float(rs.randint(1, 120))
            dets.append((im, c, float(rs.randint(0, 600)), float(rs.randint(0, 500)), w, float(rs.randint(1, 120)),
                         rs.choice([0.5, 0.25, 0.03125]) if rs.rand() < .2 else rs.randint(1, 100000) / 100000.0))
        if ii % 37 == 3:                                      # a cell with more than 100 detections, with ties
            c = cats[0]
            for k in range(130):
                dets.append((im, c, float(rs.randint(0, 300)), float(rs.randint(0, 300)), 40.0, 40.0, rs.randint(1, 40) / 100.0))
    ids = rs.permutation(len(anns) * 3)[:len(anns)] + 1        # shuffled, sparse
    ids[rs.randint(len(ids))] = 0                              # one annotation id 0
    for a, i in zip(anns, ids):
        a["id"] = int(i)
    anno = {"images": [{"id": i} for i in imgs], "categories": [{"id": c} for c in cats], "annotations": anns}
    perm = rs.permutation(len(dets))
    dets = [dets[i] for i in perm]
    return anno, dets


def as_results(dets):
    return [{"image_id": d[0], "category_id": d[1], "bbox": list(d[2:6]), "score": d[6]} for d in dets]


def batches(dets, gt_imgs, B=16):
    """Per batch of B images: (packed fp32 [rows, 7] on the device with slack rows, total, image ids); rows in detection order."""
    out = []
    for b0 in range(0, len(gt_imgs), B):
        ims = gt_imgs[b0:b0 + B]
        pos = {im: j for j, im in enumerate(ims)}
        rows = [(pos[d[0]], *d[1:]) for d in dets if d[0] in pos]
        packed = np.zeros((len(rows) + 13, 7), np.float32)
        if rows:
            packed[:len(rows)] = np.asarray(rows, np.float64)
        out.append((torch.from_numpy(packed).to(DEV), torch.tensor([len(rows)], dtype=torch.int32, device=DEV), ims))
    return out


def assert_equal(ev, ref):
    for k in ("precision", "recall", "scores"):
        assert ev.eval[k].shape == ref.eval[k].shape, k
        bad = np.argwhere(ev.eval[k] != ref.eval[k])
        assert bad.size == 0, "%s differs at %d places, first %s: %r vs %r" % (k, len(bad), bad[0].tolist(), ev.eval[k][tuple(bad[0])],
                                                                               ref.eval[k][tuple(bad[0])])
    assert ev.eval["counts"] == ref.eval["counts"]
    assert np.array_equal(np.asarray(ev.stats), ref.stats)


def run_dev(gt, feed, img_ids=None, cat_ids=None):
    ev = M.CocoEval(gt)
    feed(ev)
    if img_ids is not None:
        ev.params.imgIds = img_ids
    if cat_ids is not None:
        ev.params.catIds = cat_ids
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


@pytest.mark.parametrize("seed,str_ids", [(0, False), (1, False), (2, True)])
def test_load_res_equals_restatement(seed, str_ids):
    anno, dets = synth_set(seed, str_ids=str_ids)
    res = as_results(dets)
    ref = R.run(anno, res)
    assert (ref.eval["precision"] == -1).any() and (ref.eval["precision"] > 0).any()
    gt = M.CocoGt(anno)
    ev = run_dev(gt, lambda e: e.load_res(res))
    assert_equal(ev, ref)
    # the gt is reused: a second evaluation over narrowed images and categories
    img_ids = [im["id"] for im in anno["images"]][::3]
    cat_ids = [c["id"] for c in anno["categories"]][:12] + [5000]
    ref2 = R.CocoEvalRef(anno, res)
    ref2.params.imgIds, ref2.params.catIds = img_ids, cat_ids
    ref2.evaluate()
    ref2.accumulate()
    ref2.summarize()
    assert_equal(run_dev(gt, lambda e: e.load_res(res), img_ids, cat_ids), ref2)


def test_update_equals_load_res_and_restatement():
    anno, dets = synth_set(3)
    gt = M.CocoGt(anno)
    imgs = sorted(im["id"] for im in anno["images"])
    bs = batches(dets, imgs)
    host_rows = []
    for packed, total, ims in bs:                            # the host rounding of post.coco_results
        host_rows.extend(P.coco_results(packed, total, ["/d/%d.jpg" % i for i in ims], is_coco=True))
    ref = R.run(anno, host_rows)
    ev_u = run_dev(gt, lambda e: [e.update(p, t, ims) for p, t, ims in bs])
    ev_l = run_dev(gt, lambda e: e.load_res(host_rows))
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(ev_u.eval[k], ev_l.eval[k]), k
    assert_equal(ev_u, ref)


def test_no_results():
    anno, _ = synth_set(4, n_img=20, n_cat=5)
    ev = run_dev(M.CocoGt(anno), lambda e: None)
    assert_equal(ev, R.run(anno, []))
    assert (ev.eval["recall"] == 0).any() and (ev.eval["recall"] == -1).any()


def test_errors():
    anno, dets = synth_set(5, n_img=20, n_cat=5)
    gt = M.CocoGt(anno)
    ev = M.CocoEval(gt)
    with pytest.raises(M.MafError):
        ev.load_res([{"image_id": 99999999, "category_id": anno["categories"][0]["id"], "bbox": [0, 0, 1, 1], "score": .5}])
    with pytest.raises(M.MafError):
        ev.update(torch.zeros(4, 7, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), [99999999])
    with pytest.raises(M.MafError):
        ev.update(torch.zeros(4, 7), torch.zeros(1, dtype=torch.int32), [anno["images"][0]["id"]])
    for name, value in (("maxDets", [1, 10, 300]), ("iouThrs", np.linspace(.5, .95, 10)[:5]), ("areaRng", [[0, 1e10]] * 4),
                        ("recThrs", np.linspace(0, 1, 11)), ("useCats", 0)):
        ev = M.CocoEval(gt)
        setattr(ev.params, name, value)
        with pytest.raises(M.MafError):
            ev.evaluate()
    with pytest.raises(M.MafError):
        M.CocoGt(anno, device="cpu")
    crowded = {"images": [{"id": 1}], "categories": [{"id": 1}],
               "annotations": [{"id": i + 1, "image_id": 1, "category_id": 1, "bbox": [0, 0, 1, 1], "area": 1.0} for i in range(lib.COCO_MAX_GT + 1)]}
    with pytest.raises(M.MafError):
        M.CocoGt(crowded)


def model_n():
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", seed=0, cls_bias=-3.0))
    return m.to(DEV).eval()


def test_eval_loop_coco_metric_end_to_end(capsys):
    model = model_n()
    rs = np.random.RandomState(21)
    loader, rows_seen = [], []
    for bi, B in enumerate((4, 3)):
        imgs = torch.from_numpy(rs.randint(0, 256, (B, 3, 256, 256)).astype(np.uint8))
        shapes = [((480, 640), ((0.4, 0.4), (0.0, 32.0))), ((256, 256), ((1.0, 1.0), (0.0, 0.0))), ((333, 500), ((0.512, 0.512), (0.0, 42.75))),
                  ((640, 480), ((0.4, 0.4), (32.0, 0.0)))][:B]
        loader.append((imgs, torch.zeros(0, 6), ["/x/%012d.jpg" % (100 * bi + b) for b in range(B)], shapes))
    base = EL.EvalLoop(model, half=True, ids=list(range(80)))
    rows_plain = base.predict_model(loader)
    assert base.coco_metric_result is None and len(rows_plain) > 0
    # ground truth: jittered copies of some detections, one crowd, plus a gt-only image that the loop never sees
    anns = []
    for j, r in enumerate(rows_plain[::5]):
        x, y, w, h = r["bbox"]
        anns.append({"id": j + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": [x + 1.5, y - 1.0, w, h + 2.0],
                     "area": w * (h + 2.0), "iscrowd": int(j == 3)})
    seen = sorted({int(p.split("/")[-1][:-4]) for _, _, paths, _ in loader for p in paths})
    anno = {"images": [{"id": i} for i in seen + [777777]], "categories": [{"id": c} for c in range(80)],
            "annotations": anns + [{"id": 9999, "image_id": 777777, "category_id": 0, "bbox": [0, 0, 50, 50], "area": 2500.0}]}
    loop = EL.EvalLoop(model, half=True, ids=list(range(80)), do_coco_metric=True, anno=M.CocoGt(anno))
    rows = loop.predict_model(loader)
    assert rows == rows_plain
    ref = R.run(anno, rows, img_ids=seen)
    assert_equal(loop.coco_eval, ref)
    s = ref.stats
    assert loop.coco_metric_result == (s[1], s[0], s[2], s[3], s[4], s[5])
    assert "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in capsys.readouterr().out
    # is_coco=False: every gt image is evaluated, the one never seen included
    anno_s = {**anno, "images": [{"id": "%012d" % i} for i in seen + [777777]],
              "annotations": [{**a, "image_id": "%012d" % a["image_id"]} for a in anno["annotations"]]}
    loop2 = EL.EvalLoop(model, half=True, ids=list(range(80)), is_coco=False, do_coco_metric=True, anno=anno_s)
    rows2 = loop2.predict_model(loader)
    ref2 = R.run(anno_s, rows2)
    assert_equal(loop2.coco_eval, ref2)
    assert ref2.stats[8] != ref.stats[8]                     # the unseen image's gt counts against recall
    quiet = EL.EvalLoop(model, conf_thres=1.0, half=True, ids=list(range(80)), do_coco_metric=True, anno=M.CocoGt(anno))
    assert quiet.predict_model(loader) == [] and quiet.coco_metric_result == (0.0, 0.0)


def test_update_does_not_sync():
    anno, dets = synth_set(6, n_img=64, n_cat=8)
    gt = M.CocoGt(anno)
    bs = batches(dets, sorted(im["id"] for im in anno["images"]))
    warm = M.CocoEval(gt)                                    # library loaded, pinned pool primed
    warm.update(*bs[0])
    torch.cuda.synchronize()
    ev = M.CocoEval(gt)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, t, ims in bs:
            ev.update(p, t, ims)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ev.evaluate()
            ev.accumulate()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    syncs = [x for x in w if "synchroniz" in str(x.message)]
    assert len(syncs) == 1, [str(x.message) for x in syncs]


def test_torch_ops_match_the_c_abi_path():
    from maf_yolo_amd import cocoeval as CE
    from maf_yolo_amd import torch_ops
    ops = torch_ops.load()
    anno, dets = synth_set(7, n_img=48, n_cat=10)
    gt = M.CocoGt(anno)
    bs = batches(dets, sorted(im["id"] for im in anno["images"]))
    ev = run_dev(gt, lambda e: [e.update(p, t, ims) for p, t, ims in bs])
    for (p, t, ims), chunk in zip(bs, ev._chunks):
        idx = torch.tensor([gt.img_index[i] for i in ims], dtype=torch.int32, device=DEV)
        for a, b in zip(ops.coco_append(p, t, idx, gt.cat_lut), chunk):
            assert torch.equal(a, b)
    e = ev._ev
    iou_thrs, area_rng, box, cell_keys = e["keep"]
    I, K = gt.num_images, gt.num_categories
    rank, mbits, ibits, npig = ops.coco_match(gt.box, gt.area, gt.flags, gt.off, cell_keys, e["order"], box, e["img_sel"], e["cat_map"], I, K,
                                              iou_thrs, area_rng)
    assert torch.equal(rank, e["rank"]) and torch.equal(mbits, e["mbits"]) and torch.equal(ibits, e["ibits"])
    assert torch.equal(npig.reshape(-1), e["npig"])
    _, p3 = torch.sort(-e["score"], stable=True)
    ck = torch.where(rank >= 0, e["cat_map"][e["cat"].long().clamp(min=0)].long(), torch.full_like(e["mbits"], CE.INT64_MAX))
    cat_keys, p4 = torch.sort(ck[p3], stable=True)
    pos = p3[p4]
    d = CE._default_params()
    prec, rec, sc = ops.coco_accumulate(cat_keys, rank[pos].contiguous(), mbits[pos].contiguous(), ibits[pos].contiguous(),
                                        e["score"][pos].contiguous(), npig, e["img_sel"], e["cat_of"], I, K,
                                        torch.tensor(d["recThrs"], dtype=torch.float64, device=DEV),
                                        torch.tensor(d["maxDets"], dtype=torch.int32, device=DEV))
    assert np.array_equal(prec.cpu().numpy(), ev.eval["precision"]) and np.array_equal(rec.cpu().numpy(), ev.eval["recall"])
    assert np.array_equal(sc.cpu().numpy(), ev.eval["scores"])
