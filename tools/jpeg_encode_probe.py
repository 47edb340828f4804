"""Measurements of the JPEG encoder (csrc/jpeg_encode.hip, maf-yolo_amd/jpeg_encode.py) on the GPU; prints ONE JSON line.

    python tools/jpeg_encode_probe.py [--iters N] [--threads 16]

Two workloads, quality 95, 4:2:0:
* "frames": 32 frames of 480 x 640 (a photograph-like synthetic picture, every frame shifted so no two are equal), one file per frame;
* "crops":  32 frames x 30 rectangles of about 100 x 100 (sizes 80..120, seeded), one file per rectangle, 960 files per call.
Per workload: images/s of the device work alone (stream events around encode() after warm-up, median of `iters`; host preparation of the
call overlaps it in a pipeline and is reported beside it as the wall time of encode() with the device idle), images/s of encode() +
files() end to end (wall clock, the read-back included), the bytes read and written on the device, and the same work by Pillow on the
host with `threads` threads (Pillow releases the GIL inside libjpeg) where Pillow is importable.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maf_yolo_amd import jpeg_encode as E  # noqa: E402

DEV = torch.device("cuda:0")


def picture(h, w, shift):
    """Smooth structure + fine texture + a little noise: a file of roughly photographic size at quality 95."""
    rng = np.random.default_rng(shift)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x = x + 17 * shift
    ch = []
    for c in range(3):
        f = 128 + 70 * np.sin(x / (23.0 + 7 * c) + c) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 3.1 + c)
        f += rng.normal(0, 4 + 3 * c, (h, w))
        ch.append(np.clip(f, 0, 255))
    return np.stack(ch, -1).astype(np.uint8)


def pillow_images_per_s(crops, threads):
    try:
        from PIL import Image
    except ImportError:
        return None

    def one(bgr):
        buf = io.BytesIO()
        Image.fromarray(bgr[..., ::-1]).save(buf, "JPEG", quality=95, subsampling="4:2:0")
        return buf.tell()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, crops[:threads]))
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(one, crops))
            ts.append(time.perf_counter() - t0)
    return round(len(crops) / statistics.median(ts), 1)


def measure(frames, rects, iters):
    n = len(frames) if rects is None else len(rects)
    for _ in range(3):
        enc = E.encode(frames, 95, "4:2:0", rects=rects)
        files = enc.files()
    ts, host = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        enc = E.encode(frames, 95, "4:2:0", rects=rects)
        e1.record()
        host.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    wall = []
    for _ in range(iters):
        t0 = time.perf_counter()
        E.encode(frames, 95, "4:2:0", rects=rects).files()
        wall.append(time.perf_counter() - t0)
    taps = {}
    E.encode(frames, 95, "4:2:0", rects=rects, taps=taps).files()
    jobs = taps["jobs"]
    pixels = int((jobs["w"].astype(np.int64) * jobs["h"]).sum())
    blocks = int(taps["header"]["n_blocks"])
    out = sum(len(f) for f in files)
    t = statistics.median(ts)
    return dict(files=n, file_bytes=out, blocks=blocks,
                device_ms=round(t * 1e3, 3), images_per_s_device=round(n / t, 1),
                host_enqueue_ms=round(statistics.median(host) * 1e3, 3),
                images_per_s_end_to_end=round(n / statistics.median(wall), 1),
                bytes=dict(pixels_read=3 * 3 * pixels,                    # every pixel is fetched once per component
                           coef_write_read=128 * blocks * 3,              # written by transform, read by count and by pack
                           packed_zeroed=int(taps["header"]["n_chunks"]) * E.CHUNK,
                           files_written=out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    host = [picture(480, 640, i) for i in range(32)]
    frames = [torch.from_numpy(f).to(DEV) for f in host]
    rng = np.random.default_rng(0)
    rects = []
    for i in range(32):
        for _ in range(30):
            w, h = (int(v) for v in rng.integers(80, 121, 2))
            x, y = int(rng.integers(0, 640 - w + 1)), int(rng.integers(0, 480 - h + 1))
            rects.append((i, x, y, x + w, y + h))
    rects = np.array(rects)
    res = {"metric": "jpeg_encode_probe", "quality": 95, "subsampling": "4:2:0", "pillow_threads": args.threads}
    res["frames"] = measure(frames, None, args.iters)
    res["frames"]["images_per_s_pillow"] = pillow_images_per_s(host, args.threads)
    res["crops"] = measure(frames, rects, args.iters)
    res["crops"]["images_per_s_pillow"] = pillow_images_per_s([np.ascontiguousarray(host[i][y1:y2, x1:x2]) for i, x1, y1, x2, y2 in rects.tolist()], args.threads)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
