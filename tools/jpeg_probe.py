"""Measurements of the JPEG decoder (csrc/jpeg_decode.hip, maf-yolo_amd/jpeg.py) on the GPU; prints ONE JSON line.

    python tools/jpeg_probe.py [--iters N] [--batches 32,256,1024] [--progressive] [--orientation]

The file is the 480 x 640, 4:2:0, quality 90 case of tests/golden/jpeg_cases.npz replicated to B files per call.  Per B:
* images/s of decode(files, check=False) end to end (host parse + staging + copy + the three kernels), wall clock over `iters` calls with
  one synchronisation at the end, and of decode(files) with its status read per call;
* the host's share: wall time of a call with the device idle behind it (enqueue only);
* per-stage device times from event pairs around maf_jpeg_decode restricted to one stage (entropy includes the coefficient memset);
* bytes moved per call: file bytes copied host -> device, coefficients written + read, planes written + read, frame bytes written.
Where Pillow is importable, the single-thread Pillow decode time of the same file stands beside them.
--progressive: the same picture as a progressive file (the 480 x 640 case of tests/golden/jpeg_progressive_cases.npz: 10 scans), decoded with
progressive=True; per B additionally the launch count of a call (memsets aside: one entropy launch per scan round + IDCT + colour), the entropy
stage as a whole (the coefficient memset and all rounds, which follow each other on the stream) and its mean per round, and under "baseline"
the figures of the baseline file at the same B, measured in the same run.
--orientation: instead, the per-stage device times of the baseline file with the image table's orientation set to 1 and to 2 ... 8 (the scan
bytes are the same: only the colour kernel's final store differs), decoded frames checked against the permuted orientation-1 frame.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maf_yolo_amd import jpeg as J, lib  # noqa: E402

DEV = torch.device("cuda:0")


def stage_times(files, iters, progressive=False, orientation=0, frames=None):
    """Event time of each stage alone, on buffers a full decode has filled.  orientation: written into every image's record; frames: a list
    that receives the output buffer and the image table."""
    infos = [J.parse(f, progressive) for f in files]
    hdr, images, lanes, huff, quant, scan_at, prog = J.build_blob(files, infos)
    images["orientation"] = orientation
    stage = torch.empty(int(hdr["total_bytes"]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    J.fill_blob(host, hdr, images, lanes, huff, quant, files, infos, scan_at, prog)
    blob = stage.to(DEV)
    coef = torch.empty(int(hdr["coef_elems"]), dtype=torch.int16, device=DEV)
    planes = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=DEV)
    out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=DEV)
    status = torch.empty(len(files), dtype=torch.int32, device=DEV)
    L = lib.load()
    st = torch.cuda.current_stream(DEV)
    res = {}
    for name, mask in (("entropy", J.STAGE_ENTROPY), ("idct", J.STAGE_IDCT), ("color", J.STAGE_COLOR), ("all", J.STAGE_ALL)):
        def run():
            lib.check(L.maf_jpeg_decode(host.ctypes.data, blob.data_ptr(), coef.data_ptr(), planes.data_ptr(), out.data_ptr(), status.data_ptr(),
                                        mask, st.cuda_stream))
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name + "_us"] = round(statistics.median(ts), 1)
    if frames is not None:
        frames += [out, images]
    res["bytes"] = dict(h2d=int(hdr["total_bytes"]), coef_write_read=4 * int(hdr["coef_elems"]), planes_write_read=2 * int(hdr["plane_bytes"]),
                        frames=int(hdr["out_bytes"]), lanes=int((lanes["image"] >= 0).sum()))
    if prog is not None:
        rounds = int(hdr["n_rounds"])
        res["launches"] = (1 if len(lanes) else 0) + rounds + 2
        res["entropy_rounds"] = rounds
        res["entropy_us_per_round_mean"] = round(res["entropy_us"] / rounds, 1)
        res["bytes"]["scan_lanes"] = int((prog[1]["image"] >= 0).sum())
        res["bytes"]["lanes_per_workgroup"] = int(hdr["sgroup"])
    return res


def pillow_ms(data):
    try:
        from PIL import Image
    except ImportError:
        return None
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def measure(data, B, iters, progressive):
    files = [data] * B
    J.decode(files, device=DEV, progressive=progressive)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        J.decode(files, device=DEV, check=False, progressive=progressive)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_async = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(iters):
        J.decode(files, device=DEV, progressive=progressive)
    t_sync = time.perf_counter() - t0
    c = dict(B=B, img_s_check_false=round(B * iters / t_async, 1), img_s_check_true=round(B * iters / t_sync, 1),
             host_enqueue_ms_per_call=round(t_enq / iters * 1e3, 2))
    c.update(stage_times(files, max(3, iters), progressive))
    torch.cuda.empty_cache()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--progressive", action="store_true", help="measure the progressive encoding of the same picture (and the baseline one beside it)")
    ap.add_argument("--orientation", action="store_true", help="measure the colour stage with the EXIF orientation 1 ... 8 in the image table")
    args = ap.parse_args()
    data = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["large_file"].tobytes()
    res = {"metric": "jpeg_probe", "file": "480x640 4:2:0 q90, %d bytes" % len(data), "cases": {}}
    res["pillow_single_thread_ms"] = pillow_ms(data)
    if args.orientation:
        res["metric"] = "jpeg_probe_orientation"
        for B in [int(b) for b in args.batches.split(",")]:
            c, upright = {}, None
            for o in range(1, 9):
                got = []
                t = stage_times([data] * B, max(3, args.iters), orientation=o, frames=got)
                out, images = got
                h, w = int(images[0]["h"]), int(images[0]["w"])
                first = out[:3 * h * w].view(*((w, h, 3) if o >= 5 else (h, w, 3))).cpu()
                if o == 1:
                    upright = first
                flip = {2: lambda f: f.flip(1), 3: lambda f: f.flip(0, 1), 4: lambda f: f.flip(0), 5: lambda f: f.transpose(0, 1),
                        6: lambda f: f.flip(0).transpose(0, 1), 7: lambda f: f.flip(0, 1).transpose(0, 1), 8: lambda f: f.flip(1).transpose(0, 1)}
                assert o == 1 or torch.equal(first, flip[o](upright)), o
                c[str(o)] = {k: t[k] for k in ("entropy_us", "idct_us", "color_us", "all_us")}
            res["cases"][str(B)] = c
        print(json.dumps(res))
        return
    if args.progressive:
        pdata = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_progressive_cases.npz"))["large_file"].tobytes()
        res["metric"] = "jpeg_probe_progressive"
        res["progressive_file"] = "480x640 4:2:0 q90 progressive (10 scans), %d bytes" % len(pdata)
        res["pillow_single_thread_ms_progressive"] = pillow_ms(pdata)
    for B in [int(b) for b in args.batches.split(",")]:
        if args.progressive:
            c = measure(pdata, B, args.iters, True)
            c["baseline"] = measure(data, B, args.iters, False)
        else:
            c = measure(data, B, args.iters, False)
        res["cases"][str(B)] = c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
