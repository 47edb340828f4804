#!/usr/bin/env python3
"""Cost of the in-process mAP (maf-yolo_amd/metrics.py, csrc/pr_metric.hip) on one GPU, on a synthetic val2017-sized stream: 5000 images,
batch 32 at 640 x 640, max_det 300 (every image full: 1.5 M records), 7 labels per image, 80 classes.

    python tools/pr_metric_probe.py [--images 5000] [--model]       # one JSON line
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/pr_metric_probe.py    # kernel times of pr_match / the compute() launches

Reports, from device events: PrMetric.update per batch of 32 (one maf_pr_match launch) and compute() (stable sort + maf_pr_curves' three
launches + the copy back); with --model, the forward + NMS of MAF-YOLO-n at batch 32 (fp16, uint8 input) and what do_pr_metric adds to it;
and the NumPy restatement's host time for the same statistics (tests/pr_metric_ref.py: per image on a sample, ap_per_class on every row).
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

DEV = torch.device("cuda:0")


def stream(images, bs, nc, max_det, nl_img, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for i in range(0, images, bs):
        B = min(bs, images - i)
        nl = nl_img * B
        lxy = torch.rand(nl, 2, device=DEV, generator=g) * 500
        lwh = torch.rand(nl, 2, device=DEV, generator=g) * 120 + 8
        lcls = torch.randint(0, nc, (nl,), device=DEV, generator=g).float()
        img = torch.arange(B, device=DEV).repeat_interleave(nl_img).float()
        targets = torch.cat([img[:, None], lcls[:, None], (lxy + lwh / 2) / 640, lwh / 640], 1).contiguous()
        src = torch.randint(0, nl_img, (B, max_det), device=DEV, generator=g) + torch.arange(B, device=DEV)[:, None] * nl_img
        box = torch.cat([lxy, lxy + lwh], 1)[src] + torch.randn(B, max_det, 4, device=DEV, generator=g) * 10
        box[..., 2:] = torch.maximum(box[..., 2:], box[..., :2] + 1)
        cls = torch.where(torch.rand(B, max_det, device=DEV, generator=g) < 0.7, lcls[src],
                          torch.randint(0, nc, (B, max_det), device=DEV, generator=g).float())
        conf = (torch.rand(B, max_det, device=DEV, generator=g) * 0.97 + 0.03).half().float()
        rows = torch.cat([box, conf[..., None], cls[..., None]], 2).contiguous()
        out.append((rows, torch.full((B,), max_det, dtype=torch.int32, device=DEV), targets))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--model", action="store_true", help="also time MAF-YOLO-n forward + NMS with and without the metric")
    ap.add_argument("--host", action="store_true", help="also time the NumPy restatement")
    a = ap.parse_args()
    shapes = [((480, 640), ((1.0, 1.0), (0.0, 80.0)))] * a.bs
    data = stream(a.images, a.bs, 80, 300, 7, 1)
    res = {"images": a.images, "bs": a.bs, "max_det": 300, "labels_per_image": 7, "nc": 80}
    for rep in range(2):                                    # rep 0 warms (library, allocator, pinned pool)
        pm = M.PrMetric(80, confusion=True)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(data) + 2)]
        ev[0].record()
        for i, (rows, cnt, tg) in enumerate(data):
            pm.update(rows, cnt, tg, (640, 640), shapes[:rows.shape[0]])
            ev[i + 1].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pm.compute()
        t_compute = time.perf_counter() - t0
        per = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(data))]
    res.update(update_ms_per_batch_median=float(np.median(per)), update_ms_total=float(np.sum(per)), compute_ms=1e3 * t_compute,
               records=int(pm.bound), map50=out.map50, map=out.map)
    if a.model:
        from oracle import maf_oracle as O
        m = M.Model("n")
        m.load_state_dict(O.synth_state_dict("n", 0))                # the weights smoke() and the bench use
        m = m.to(DEV).eval().half()
        m.precision = "fp16"
        x = torch.randint(0, 256, (a.bs, 3, 640, 640), dtype=torch.uint8, device=DEV)
        tg = data[0][2]
        pm = M.PrMetric(80)
        times = {"off": [], "on": []}
        with torch.no_grad():
            for it in range(60):
                for mode in ("off", "on"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pred = m(x)[0]
                    rows, _, cnt = M.nms_raw(pred, 0.03, 0.65, multi_label=True)
                    if mode == "on":
                        pm.update(rows, cnt, tg, (640, 640), shapes)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 10:
                        times[mode].append(e0.elapsed_time(e1))
        off, on = float(np.median(times["off"])), float(np.median(times["on"]))
        res.update(fwd_nms_ms=off, fwd_nms_pr_ms=on, pr_added_pct=100.0 * (on - off) / off)
    if a.host:
        import pr_metric_ref as R
        ref = R.PrMetricRef(80)
        sample = data[:4]
        t0 = time.perf_counter()
        for rows, cnt, tg in sample:
            ref.update(rows.cpu().numpy(), cnt.cpu().numpy(), tg.cpu().numpy(), (640, 640), shapes[:rows.shape[0]])
        per_img = (time.perf_counter() - t0) / sum(int(r.shape[0]) for r, _, _ in sample)
        tp = np.random.RandomState(0).rand(a.images * 300, 10) < 0.3
        conf = np.random.RandomState(1).rand(tp.shape[0]).astype(np.float32)
        pcls = np.random.RandomState(2).randint(0, 80, tp.shape[0]).astype(np.float64)
        tcls = np.random.RandomState(3).randint(0, 80, a.images * 7).astype(np.float64)
        t0 = time.perf_counter()
        R.ap_per_class(tp, conf, pcls, tcls)
        res.update(host_ms_per_image=1e3 * per_img, host_ap_per_class_s=time.perf_counter() - t0, host_threads=torch.get_num_threads())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
