"""Measurements of the lossy WebP decoder (csrc/vp8_decode.hip, maf-yolo_amd/webp_lossy.py) on the GPU; prints ONE JSON line and writes it to
profiles/webp_lossy_probe.json.

    python tools/webp_lossy_probe.py [--iters N] [--batches 32,64] [--quality 80] [--method 4]

The file is the 480 x 640 picture of tests/golden/jpeg_cases.npz (its large case, decoded by Pillow) re-encoded by Pillow as a lossy WebP
file and replicated to B files per call (the decode of one of them is first compared with Pillow's, bit for bit).  Per B (32, and 64 to see
whether the parse stage's time stays flat while every file still has a wave of its own):
* images/s of decode(files, check=False) end to end (host parse + staging + copy + the four kernels), wall clock over `iters` calls with
  one synchronisation at the end, and of decode(files) with its status read per call;
* the host's share: wall time of parse + build_blob + fill_blob for the call, and of a call with the device idle behind it (enqueue only);
* per-stage device times from event pairs around maf_vp8_decode restricted to one stage (on buffers a full decode has filled), and the
  parse stage's time per file when every file of the call has a wave of its own (B = 32: the per-stream rate);
* bytes moved per call, the scratch included.
The single-thread Pillow (libwebp) decode time of the same file on the same host stands beside them.
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
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maf_yolo_amd import lib, webp_lossy as W  # noqa: E402

DEV = torch.device("cuda:0")
STAGES = (("all", W.STAGE_ALL), ("parse", W.STAGE_PARSE), ("recon", W.STAGE_RECON), ("filter", W.STAGE_FILTER), ("convert", W.STAGE_CONVERT))


def host_ms(files):
    t0 = time.perf_counter()
    infos = [W.parse(f) for f in files]
    hdr, images = W.build_blob(infos)
    buf = np.empty(int(hdr["total_bytes"]), np.uint8)
    W.fill_blob(buf, hdr, images, files, infos)
    return round((time.perf_counter() - t0) * 1e3, 2)


def stage_times(files, iters):
    """Event time of each stage alone, on buffers a full decode has filled."""
    infos = [W.parse(f) for f in files]
    hdr, images = W.build_blob(infos)
    stage = torch.empty(int(hdr["total_bytes"]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    W.fill_blob(host, hdr, images, files, infos)
    blob = stage.to(DEV)
    scratch = torch.empty(int(hdr["scratch_bytes"]), dtype=torch.uint8, device=DEV)
    recon = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=DEV)
    yuv = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=DEV)
    out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=DEV)
    status = torch.empty(len(files), dtype=torch.int32, device=DEV)
    L = W._library()
    st = torch.cuda.current_stream(DEV)
    res = {}
    for name, mask in STAGES:
        def run():
            lib.check(L.maf_vp8_decode(host.ctypes.data, blob.data_ptr(), scratch.data_ptr(), recon.data_ptr(), yuv.data_ptr(), out.data_ptr(),
                                       status.data_ptr(), mask, st.cuda_stream))
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name + "_us"] = round(statistics.median(ts), 1)
    assert int(status.abs().sum()) == 0
    res["bytes"] = dict(h2d=int(hdr["total_bytes"]), scratch=int(hdr["scratch_bytes"]), planes=2 * int(hdr["plane_bytes"]), frames=int(hdr["out_bytes"]))
    return res


def pillow_ms(data):
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def measure(data, B, iters):
    files = [data] * B
    W.decode(files, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        W.decode(files, device=DEV, check=False)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_async = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(iters):
        W.decode(files, device=DEV)
    t_sync = time.perf_counter() - t0
    c = dict(B=B, img_s_check_false=round(B * iters / t_async, 1), img_s_check_true=round(B * iters / t_sync, 1),
             host_enqueue_ms_per_call=round(t_enq / iters * 1e3, 2), host_parse_staging_ms_per_call=host_ms(files))
    c.update(stage_times(files, max(3, iters)))
    torch.cuda.empty_cache()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batches", default="32,64")
    ap.add_argument("--quality", type=int, default=80)
    ap.add_argument("--method", type=int, default=4, help="the writer's effort (Pillow's method, 0 .. 6)")
    args = ap.parse_args()
    jpg = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["large_file"].tobytes()
    buf = io.BytesIO()
    Image.open(io.BytesIO(jpg)).convert("RGB").save(buf, "WEBP", quality=args.quality, method=args.method)
    data = buf.getvalue()
    info = W.parse(data)
    want = torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))[:, :, 2::-1]))
    assert torch.equal(W.decode([data], device=DEV)[0].cpu(), want)
    res = {"metric": "webp_lossy_probe", "file": "%dx%d RGB lossy, written by Pillow (quality %d, method %d), %d bytes" %
           (info.height, info.width, args.quality, args.method, len(data)), "pillow_single_thread_ms": pillow_ms(data), "cases": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        res["cases"][str(B)] = measure(data, B, args.iters)
    res["pillow_single_thread_img_s"] = round(1e3 / res["pillow_single_thread_ms"], 1)
    first = res["cases"][args.batches.split(",")[0]]
    res["parse_ms_per_file_one_wave_each"] = round(first["parse_us"] / 1e3, 3)        # B <= the chip's free workgroup slots: the time of one stream
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "webp_lossy_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
