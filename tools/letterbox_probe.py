"""Measurements of the letterbox layer (csrc/letterbox.hip) on the GPU; prints ONE JSON line.

    python tools/letterbox_probe.py [--iters N] [--no-e2e] [--no-torch]

* per case (32 x 1080p -> 384 x 640, 32 x 720p -> 384 x 640 (area-fast), 32 x 480 x 640 -> 480 x 640 (copy + pad)): several distinct frame
  batches (> 256 MiB in all, so the reads come from HBM, not the Infinity Cache) rotated through the timed loop; event time per batch, the
  algorithmic bytes (source rows the filter touches x 3 w, plus 3 H W of output per image), TB/s and the fraction of the 8 TB/s spec.  Kernel
  times proper come from a rocprofv3 --kernel-trace --stats run of this same script (the kernel is `letterbox_kernel`);
* the same integer rule composed of torch ops on the GPU (gathers + integer arithmetic), timed as the baseline and compared bit for bit;
* end to end, same process, alternating, median of 5: frames -> detections (detect_frames) against forward + NMS of the already
  letterboxed uint8 batch, MAF-YOLO-n at batch 32 with the tuned plan bench.py loads (profiles/round6_tune.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maf_yolo_amd as M  # noqa: E402
import importlib  # noqa: E402

LB = importlib.import_module("maf_yolo_amd.letterbox")
HBM_PEAK = 8e12
DEV = torch.device("cuda:0")


def rows_touched(h, nh):
    """Distinct source rows the vertical filter reads for an h -> nh resize (the restatement's row rule)."""
    if h == nh:
        return h
    if h == 2 * nh:
        return h
    scale = 1.0 / (nh / h)
    f = ((np.arange(nh) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    fq = np.rint((f - s.astype(np.float32)) * np.float32(2048)).astype(np.int64)
    r = set(np.clip(s, 0, h - 1).tolist()) | set(np.clip(s + 1, 0, h - 1)[fq > 0].tolist())
    return len(r)


def torch_rule(frames, geoms, H, W, color=(114, 114, 114)):
    """The restatement's integer rule as torch ops on the GPU (the baseline)."""
    out = torch.empty(len(frames), 3, H, W, dtype=torch.uint8, device=frames[0].device)
    for b, (f, g) in enumerate(zip(frames, geoms)):
        nw, nh = g["new_unpad"]
        h, w = f.shape[:2]
        out[b] = torch.tensor(color[::-1], dtype=torch.uint8, device=f.device).view(3, 1, 1)
        s = f.to(torch.int32)
        if (w, h) == (nw, nh):
            im = s
        elif w == 2 * nw and h == 2 * nh:
            im = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        else:
            def coef(n_dst, n_src, clamp):
                f_ = ((torch.arange(n_dst, dtype=torch.float64, device=f.device) + 0.5) * (1.0 / (n_dst / n_src)) - 0.5).float()
                s_ = torch.floor(f_)
                f_ = f_ - s_
                s_ = s_.long()
                if clamp:
                    f_ = torch.where((s_ < 0) | (s_ >= n_src - 1), torch.zeros_like(f_), f_)
                    s_ = s_.clamp(0, n_src - 1)
                return s_, torch.round((1 - f_) * 2048).int(), torch.round(f_ * 2048).int()
            sx, a0, a1 = coef(nw, w, True)
            hor = s[:, sx] * a0.view(1, -1, 1) + s[:, (sx + 1).clamp(max=w - 1)] * a1.view(1, -1, 1)
            sy, b0, b1 = coef(nh, h, False)
            S0, S1 = hor[sy.clamp(0, h - 1)], hor[(sy + 1).clamp(0, h - 1)]
            im = ((((S0 >> 4) * b0.view(-1, 1, 1)) >> 16) + (((S1 >> 4) * b1.view(-1, 1, 1)) >> 16) + 2) >> 2
            im = im.clamp(0, 255)
        out[b, :, g["top"]:g["top"] + nh, g["left"]:g["left"] + nw] = im.to(torch.uint8).permute(2, 0, 1).flip(0)
    return out


def time_ms(fn, batches, iters):
    for bt in batches:
        fn(bt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch-ops baseline out (counter runs: only the kernel's dispatches)")
    args = ap.parse_args()
    res = {"metric": "letterbox_probe", "cases": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, (h, w), nb in (("1080p", (1080, 1920), 3), ("720p", (720, 1280), 4), ("480x640", (480, 640), 10)):
        B = 32
        batches = [torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device=DEV, generator=g) for _ in range(nb)]
        geo = LB.letterbox_geometry(h, w, (640, 640), True, True, 32)
        H, W = geo["shape"]
        nw, nh = geo["new_unpad"]
        byts = B * (rows_touched(h, nh) * 3 * w + 3 * H * W)
        ms = time_ms(lambda x: M.letterbox(x, 640), batches, args.iters)
        tms, same = float("nan"), None
        if not args.no_torch:
            tms = time_ms(lambda x: torch_rule(list(x.unbind(0)), [geo] * B, H, W), batches, max(3, args.iters // 10))
            same = all(torch.equal(M.letterbox(x, 640)[0], torch_rule(list(x.unbind(0)), [geo] * B, H, W)) for x in batches[:2])
        res["cases"][name] = dict(B=B, src=[h, w], out=[H, W], rotated_batches=nb, input_MiB=round(nb * B * h * w * 3 / 2**20, 1),
                                  algorithmic_MB=round(byts / 1e6, 2), event_us_per_batch=round(ms * 1e3, 2), TBps=round(byts / (ms * 1e-3) / 1e12, 3),
                                  frac_of_8TBps=round(byts / (ms * 1e-3) / HBM_PEAK, 3), torch_ops_us_per_batch=round(tms * 1e3, 1),
                                  torch_ops_bit_exact=bool(same))
        del batches
        torch.cuda.empty_cache()
    if not args.no_e2e:
        from maf_yolo_amd import engine as _engine
        tune = os.path.join(ROOT, "profiles", "round6_tune.json")
        if os.path.exists(tune):
            _engine.load_tune_cache(tune)
        model = M.Model("n")
        model.load_state_dict(M.synth.synth_state_dict(model, "n", 0))
        model = model.to(DEV).eval()
        model.autotune = True
        B = 32
        frames = [torch.randint(0, 256, (B, 720, 1280, 3), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]
        boxed = [M.letterbox(f, 640)[0] for f in frames]

        def e2e(i):
            return M.detect_frames(model, frames[i % 2], 640, conf_thres=0.25)

        def fwd(i):
            with torch.no_grad():
                return M.non_max_suppression(model(boxed[i % 2])[0], 0.25, 0.45, max_det=1000)

        for f in (e2e, fwd):
            for i in range(6):
                f(i)
        torch.cuda.synchronize()
        ra, rb = [], []
        n = 20
        for rep in range(5):
            for fn, acc in ((e2e, ra), (fwd, rb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    fn(i)
                torch.cuda.synchronize()
                acc.append(B * n / (time.perf_counter() - t0))
        a, b = statistics.median(ra), statistics.median(rb)
        # where the gap goes: host time of the two added Python calls (enqueue only, the GPU idle behind a synchronous NMS as in the loop above)
        # and the device-side span of each call (an event pair around it after a synchronise: kernel time, or the enqueue time where that is longer;
        # the kernel time alone comes from the kernel trace)
        host_lb, host_rs, dev_lb, dev_rs = [], [], [], []
        with torch.no_grad():
            rows, idx, cnt = M.nms_raw(model(boxed[0])[0], 0.25, 0.45, max_det=1000)
        src = [(720, 1280)] * B
        for i in range(40):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.letterbox(frames[i % 2], 640)
            host_lb.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            LB._rescale(rows, cnt, (384, 640), src, True)
            host_rs.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            for fn, acc in ((lambda: M.letterbox(frames[i % 2], 640), dev_lb), (lambda: LB._rescale(rows, cnt, (384, 640), src, True), dev_rs)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1) * 1e3)
        med = lambda v: round(statistics.median(v), 1)
        per_batch_gap_us = (B / a - B / b) * 1e6
        res["e2e"] = dict(workload="MAF-YOLO-n, 32 x 720p frames -> 384 x 640, conf 0.25", frames_to_dets_img_s=round(a, 1),
                          letterboxed_fwd_nms_img_s=round(b, 1), overhead_pct=round(100 * (b / a - 1), 2), gap_us_per_batch=round(per_batch_gap_us, 1),
                          host_us_letterbox_call=med([v * 1e6 for v in host_lb]), host_us_rescale_call=med([v * 1e6 for v in host_rs]),
                          events_us_letterbox_call=med(dev_lb), events_us_rescale_call=med(dev_rs), runs=[[round(v, 1) for v in ra], [round(v, 1) for v in rb]])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
