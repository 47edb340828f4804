"""Times CocoEval.evaluate() + accumulate() on the device at the val2017 size: 5 000 images, ~37 k gts over 80 categories with COCO's
non-contiguous ids, 300 detections per image (1.5 M), fed per batch of 32 through update() as post.coco_rows hands them over.  Events on
the stream plus one synchronise; kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/cocoeval_probe.py` run.
It also times the NumPy restatement (tests/cocoeval_ref.py) on the host at a size it finishes in reasonable time; that is the restatement's
time, not pycocotools'.

    python tools/cocoeval_probe.py [--images 5000] [--dets 300] [--reps 5] [--ref-images 100] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maf_yolo_amd as M  # noqa: E402

COCO91 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35, 36, 37, 38, 39,
          40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 70, 72, 73, 74, 75, 76, 77,
          78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90]


def synth(n_img, dets_per_img, seed=0):
    """-> (anno dict, dets [n, 7] fp32: image index, category id, x, y, w, h, score).  Category 1 (person) takes ~30 % of everything."""
    rs = np.random.RandomState(seed)
    prob = np.full(80, 0.7 / 79)
    prob[0] = 0.3
    anns, dets = [], []
    aid = 1
    for i in range(n_img):
        ng = rs.poisson(7.3)
        cats = rs.choice(80, ng, p=prob)
        xy = rs.uniform(0, 560, (ng, 2))
        wh = np.exp(rs.uniform(np.log(4), np.log(400), (ng, 2)))
        for k in range(ng):
            bb = [float(xy[k, 0]), float(xy[k, 1]), float(wh[k, 0]), float(wh[k, 1])]
            anns.append({"id": aid, "image_id": i + 1, "category_id": COCO91[cats[k]], "bbox": bb, "area": bb[2] * bb[3] * 0.8,
                         "iscrowd": int(rs.rand() < 0.01)})
            aid += 1
        nd = dets_per_img
        d = np.empty((nd, 7), np.float64)
        d[:, 0] = 0
        d[:, 1] = np.asarray(COCO91)[rs.choice(80, nd, p=prob)]
        near = rs.rand(nd) < 0.3
        d[:, 2:4] = rs.uniform(0, 560, (nd, 2))
        d[:, 4:6] = np.exp(rs.uniform(np.log(4), np.log(400), (nd, 2)))
        if ng:
            src = rs.randint(0, ng, nd)
            base = np.asarray([a["bbox"] for a in anns[-ng:]])[src]
            d[near, 2:6] = base[near] + rs.normal(0, 3, (int(near.sum()), 4))
            d[near, 1] = np.asarray([a["category_id"] for a in anns[-ng:]])[src][near]
        d[:, 4:6] = np.abs(d[:, 4:6])
        d[:, 6] = np.sort(rs.uniform(0.03, 1.0, nd))[::-1]
        dets.append(d.astype(np.float32))
    anno = {"images": [{"id": i + 1} for i in range(n_img)], "categories": [{"id": c} for c in COCO91], "annotations": anns}
    return anno, dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    anno, dets = synth(a.images, a.dets)
    t0 = time.perf_counter()
    gt = M.CocoGt(anno)
    t_gt = time.perf_counter() - t0
    feed = []
    for b0 in range(0, a.images, a.batch):
        blk = dets[b0:b0 + a.batch]
        packed = np.concatenate([np.concatenate([np.full((len(d), 1), j, np.float32), d[:, 1:]], 1) for j, d in enumerate(blk)])
        feed.append((torch.from_numpy(packed).to(dev), torch.tensor([len(packed)], dtype=torch.int32, device=dev),
                     list(range(b0 + 1, b0 + len(blk) + 1))))
    times, upd = [], []
    import contextlib
    import io
    for rep in range(a.reps + 1):
        ev = M.CocoEval(gt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p, t, ims in feed:
            ev.update(p, t, ims)
        torch.cuda.synchronize()
        upd.append(1e3 * (time.perf_counter() - t0))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        ev.evaluate()
        ev.accumulate()                                      # ends in the one device -> host copy
        e1.record()
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        if rep:
            times.append((e0.elapsed_time(e1), wall))
        with contextlib.redirect_stdout(io.StringIO()):
            ev.summarize()
    ev_ms = [t[0] for t in times]
    wall_ms = [t[1] for t in times]
    out = {"images": a.images, "gts": len(anno["annotations"]), "detections": int(sum(len(d) for d in dets)),
           "evaluate_accumulate_ms_events": {"median": float(np.median(ev_ms)), "min": float(np.min(ev_ms)), "max": float(np.max(ev_ms))},
           "evaluate_accumulate_ms_wall": {"median": float(np.median(wall_ms)), "min": float(np.min(wall_ms))},
           "update_all_batches_ms_median": float(np.median(upd[1:])) if len(upd) > 1 else upd[0], "cocogt_build_s": t_gt,
           "stats": [float(x) for x in ev.stats]}
    if a.ref_images:
        import cocoeval_ref as R
        small, sdets = synth(a.ref_images, a.dets, seed=1)
        rows = [{"image_id": i + 1, "category_id": int(r[1]), "bbox": [float(v) for v in np.round(r[2:6].astype(np.float64) * 1e3) / 1e3],
                 "score": float(np.round(np.float64(r[6]) * 1e5) / 1e5)} for i, d in enumerate(sdets) for r in d]
        t0 = time.perf_counter()
        ref = R.CocoEvalRef(small, rows)
        ref.evaluate()
        ref.accumulate()
        out["restatement_host_s"] = {"images": a.ref_images, "detections": len(rows), "evaluate_accumulate_s": time.perf_counter() - t0}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
