"""Measurements of the lossless WebP encoder (csrc/webp_encode.hip, maf-yolo_amd/webp_encode.py) on the GPU; prints ONE JSON line.  No gate.

    python tools/webp_encode_probe.py [--iters N]
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/webp_encode_probe.py --once photo

32 frames of 480 x 640 per call, predictor_bits 4, with three kinds of content: `flat` (one colour per frame), `photo` (a smooth synthetic
picture with a little noise, every frame shifted; tools/png_encode_probe.py's) and `noise`.  Per kind: milliseconds per call of the device
work alone (stream events around encode() after warm-up, median of `iters`) for webp_encode.encode and, alternating with it in the same loop,
for png_encode.encode on the same frames; the wall time of the host's part of encode(); the total size of the files, beside png_encode's
and beside Pillow's lossless=True, method=0, quality=0 (libwebp on the host; its time is not measured).  Every device file is decoded by Pillow
and compared with its frame before anything is timed.  --once KIND only encodes one batch of that kind five times: the run to put under
rocprofv3 for the time of every kernel.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from maf_yolo_amd import png_encode, webp_encode  # noqa: E402
from png_encode_probe import picture  # noqa: E402

DEV = torch.device("cuda:0")
BATCH = 32


def pillow_lossless_bytes(host):
    from PIL import Image
    total = 0
    for f in host:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, "WEBP", lossless=True, method=0, quality=0)
        total += buf.tell()
    return total


def check(files, host):
    from PIL import Image
    for data, f in zip(files, host):
        if not np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1], f):
            raise SystemExit("a device file does not decode to its frame")


def measure(frames, iters):
    encoders = {"webp": webp_encode.encode, "png": png_encode.encode}
    for enc in encoders.values():
        for _ in range(2):
            enc(frames).files()
    ts, host = {k: [] for k in encoders}, {k: [] for k in encoders}
    for _ in range(iters):
        for k, enc in encoders.items():                                         # alternating: both see the same machine
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = enc(frames)
            e1.record()
            host[k].append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
            del out
    return {k: dict(device_ms=round(statistics.median(ts[k]), 3), device_ms_min_max=[round(min(ts[k]), 3), round(max(ts[k]), 3)],
                    host_enqueue_ms=round(statistics.median(host[k]) * 1e3, 3)) for k in encoders}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--once", choices=("flat", "photo", "noise"))
    args = ap.parse_args()
    if args.once:
        frames = [torch.from_numpy(picture(args.once, i)).to(DEV) for i in range(BATCH)]
        for _ in range(5):
            n = sum(len(f) for f in webp_encode.encode(frames).files())
        print(json.dumps({"metric": "webp_encode_probe_once", "kind": args.once, "files": BATCH, "file_bytes": n}))
        return
    res = {"metric": "webp_encode_probe", "frame": [480, 640], "files_per_call": BATCH, "predictor_bits": 4, "iters": args.iters}
    for kind in ("flat", "photo", "noise"):
        host = [picture(kind, i) for i in range(BATCH)]
        frames = [torch.from_numpy(f).to(DEV) for f in host]
        files = webp_encode.encode(frames).files()
        check(files, host)
        res[kind] = measure(frames, args.iters)
        res[kind]["webp"]["file_bytes"] = sum(len(f) for f in files)
        res[kind]["png"]["file_bytes"] = sum(len(f) for f in png_encode.encode(frames).files())
        res[kind]["pillow_lossless_m0_q0_file_bytes"] = pillow_lossless_bytes(host)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
