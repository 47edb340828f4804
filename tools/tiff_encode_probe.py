"""Measurements of the TIFF encoder (csrc/tiff_encode.hip, maf-yolo_amd/tiff_encode.py) on the GPU; prints ONE JSON line.

    python tools/tiff_encode_probe.py [--iters N] [--threads 16]
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/tiff_encode_probe.py --once photo

Two batches, 32 frames of 640 x 640 (5120 strips of 7680 bytes under the cv2 strip rule) and 4 frames of 2160 x 3840 (a row is wider than
8192 bytes: 8640 strips of one row), with three kinds of content: `flat` (one colour per frame), `photo` (a smooth synthetic picture with a
little noise, every frame shifted) and `noise`.  Per batch and kind: strips per call, bytes out, files/s and MB/s of raw bytes of the device
work alone (stream events around encode() after warm-up, median of `iters`), the wall time of the host's part of encode(), files/s of
encode() + files() end to end; and, where Pillow with libtiff imports, libtiff on the host beside it on the same frames at the same settings
(Image.save, compression tiff_lzw, Predictor 2, the same RowsPerStrip; `threads` threads).  --once KIND only encodes the 32-frame batch of
that kind five times: the run to put under rocprofv3 for the time of every kernel.
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
from maf_yolo_amd import tiff_encode as E  # noqa: E402

DEV = torch.device("cuda:0")
BATCHES = {"32x640x640": (32, 640, 640), "4x2160x3840": (4, 2160, 3840)}


def picture(kind, shift, h, w):
    rng = np.random.default_rng(shift)
    if kind == "flat":
        return np.full((h, w, 3), rng.integers(0, 256, 3, dtype=np.uint8), np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    x = x + 17 * shift
    ch = [128 + 70 * np.sin(x / (23.0 + 7 * c) + c) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 3.1 + c) + rng.normal(0, 1 + c, (h, w)) for c in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def host_libtiff_files_per_s(frames, threads):
    """Pillow / libtiff on the same frames, or None where it does not import."""
    try:
        from PIL import Image, features
    except ImportError:
        return None
    if not features.check("libtiff"):
        return None
    images = [(Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])), int(E.cv2_rows_per_strip(f.shape[1], f.shape[0]))) for f in frames]

    def one(job):
        buf = io.BytesIO()
        job[0].save(buf, "TIFF", compression="tiff_lzw", tiffinfo={317: 2, 278: job[1]})
        return buf.tell()
    with ThreadPoolExecutor(threads) as pool:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(one, images))
            ts.append(time.perf_counter() - t0)
    return round(len(images) / statistics.median(ts), 1)


def measure(frames, iters):
    n = len(frames)
    taps = {}
    for _ in range(2):
        files = E.encode(frames, taps=taps).files()
    strips = int(taps["header"]["n_strips"])
    taps.clear()
    ts, host = [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        enc = E.encode(frames)
        e1.record()
        host.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
        del enc
    wall = []
    for _ in range(max(2, iters // 2)):
        t0 = time.perf_counter()
        E.encode(frames).files()
        wall.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    raw_mb = sum(3 * f.shape[0] * f.shape[1] for f in frames) / 1e6
    return dict(files=n, strips_per_call=strips, bytes_out=sum(len(f) for f in files), device_ms=round(t * 1e3, 3), files_per_s_device=round(n / t, 1),
                raw_MB_per_s_device=round(raw_mb / t, 1), host_enqueue_ms=round(statistics.median(host) * 1e3, 3),
                files_per_s_end_to_end=round(n / statistics.median(wall), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--once", choices=("flat", "photo", "noise"))
    args = ap.parse_args()
    if args.once:
        frames = [torch.from_numpy(picture(args.once, i, 640, 640)).to(DEV) for i in range(32)]
        for _ in range(5):
            n = sum(len(f) for f in E.encode(frames).files())
        print(json.dumps({"metric": "tiff_encode_probe_once", "kind": args.once, "files": 32, "bytes_out": n}))
        return
    res = {"metric": "tiff_encode_probe", "libtiff_threads": args.threads}
    for kind in ("flat", "photo", "noise"):
        res[kind] = {}
        for name, (b, h, w) in BATCHES.items():
            host = [picture(kind, i, h, w) for i in range(b)]
            got = measure([torch.from_numpy(f).to(DEV) for f in host], args.iters)
            got["files_per_s_host_libtiff"] = host_libtiff_files_per_s(host, args.threads)
            res[kind][name] = got
    print(json.dumps(res))


if __name__ == "__main__":
    main()
