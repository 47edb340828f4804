"""Measurements of the PNG encoder (csrc/png_encode.hip, maf-yolo_amd/png_encode.py) on the GPU; prints ONE JSON line.

    python tools/png_encode_probe.py [--iters N] [--threads 16]
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/png_encode_probe.py --once photo

Frames of 480 x 640, filter sub, in batches of 1, 32 and 256, with three kinds of content: `flat` (one colour per frame: long runs), `photo`
(a smooth synthetic picture with a little noise, every frame shifted: dynamic blocks) and `noise` (stored blocks).  Per batch and kind: files/s
and MB/s of filtered bytes of the device work alone (stream events around encode() after warm-up, median of `iters`), the wall time of the
host's part of encode(), files/s of encode() + files() end to end, the size of the files, and beside it the host's zlib at the same settings
(zlib.compressobj(1, DEFLATED, 15, 8, Z_RLE) over the filtered rows, which NumPy prepares outside the timing; `threads` threads — zlib releases
the GIL).  --once KIND only encodes one 32-frame batch of that kind five times: the run to put under rocprofv3 for the time of every kernel.
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maf_yolo_amd import png_encode as E  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 480, 640


def picture(kind, shift):
    rng = np.random.default_rng(shift)
    if kind == "flat":
        return np.full((H, W, 3), rng.integers(0, 256, 3, dtype=np.uint8), np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x = x + 17 * shift
    ch = [128 + 70 * np.sin(x / (23.0 + 7 * c) + c) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 3.1 + c) + rng.normal(0, 1 + c, (H, W)) for c in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def sub_filtered(bgr):
    rgb = bgr[..., ::-1].astype(np.int16)
    d = rgb.copy()
    d[:, 1:] -= rgb[:, :-1]
    return np.concatenate([np.ones((H, 1), np.uint8), d.astype(np.uint8).reshape(H, 3 * W)], 1).tobytes()


def host_zlib_files_per_s(raws, threads):
    def one(raw):
        co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        return len(co.compress(raw)) + len(co.flush())
    with ThreadPoolExecutor(threads) as pool:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(one, raws))
            ts.append(time.perf_counter() - t0)
    return round(len(raws) / statistics.median(ts), 1)


def measure(frames, iters):
    n = len(frames)
    for _ in range(2):
        files = E.encode(frames).files()
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
    raw_mb = n * H * (1 + 3 * W) / 1e6
    return dict(files=n, file_bytes=sum(len(f) for f in files), device_ms=round(t * 1e3, 3), files_per_s_device=round(n / t, 1),
                filtered_MB_per_s_device=round(raw_mb / t, 1), host_enqueue_ms=round(statistics.median(host) * 1e3, 3),
                files_per_s_end_to_end=round(n / statistics.median(wall), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--once", choices=("flat", "photo", "noise"))
    args = ap.parse_args()
    if args.once:
        frames = [torch.from_numpy(picture(args.once, i)).to(DEV) for i in range(32)]
        for _ in range(5):
            n = sum(len(f) for f in E.encode(frames).files())
        print(json.dumps({"metric": "png_encode_probe_once", "kind": args.once, "files": 32, "file_bytes": n}))
        return
    res = {"metric": "png_encode_probe", "frame": [H, W], "filter": "sub", "zlib": zlib.ZLIB_RUNTIME_VERSION, "zlib_threads": args.threads}
    for kind in ("flat", "photo", "noise"):
        host = [picture(kind, i) for i in range(32)]
        dev = [torch.from_numpy(f).to(DEV) for f in host]
        res[kind] = {}
        for b in (1, 32, 256):
            frames = [dev[i % 32] for i in range(b)]
            res[kind]["batch_%d" % b] = measure(frames, args.iters if b < 256 else max(3, args.iters // 3))
        raws = [sub_filtered(f) for f in host]
        res[kind]["files_per_s_host_zlib"] = host_zlib_files_per_s(raws, args.threads)
        res[kind]["files_per_s_host_zlib_1_thread"] = host_zlib_files_per_s(raws[:8], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
