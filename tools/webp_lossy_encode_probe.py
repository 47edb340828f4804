"""Measurements of the lossy WebP encoder (csrc/vp8_encode.hip, maf-yolo_amd/webp_lossy_encode.py); prints ONE JSON line.  No gate.

    python tools/webp_lossy_encode_probe.py [--iters N]          on the GPU: time
    python tools/webp_lossy_encode_probe.py --rd                 on the CPU: rate-distortion through the rule book (the device's bytes are its bytes)
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/webp_lossy_encode_probe.py --once

Time: 32 frames of 480 x 640 (`photo`: a smooth synthetic picture with a little noise, every frame shifted; tools/png_encode_probe.py's) and 256
crops of 64 x 64 out of them, quality 75.  Per workload milliseconds per call of the device work alone (stream events around encode() after
warm-up, median of `iters`) for webp_lossy_encode.encode and, alternating with it in the same loop, for jpeg_encode.encode and
webp_encode.encode on the same input; the wall time of the host's part of encode(); the total size of the files.  The first file of every call
is decoded by Pillow and by webp_lossy.decode and the two are compared before anything is timed.

--rd: three 96 x 64 frames (smooth, photo, hard edges) at base_q 10, 40 and 80: bytes and the BGR PSNR of Pillow's decode, with the default
filter level and with level 0; next to them the PSNR of Pillow's own WebP (method 4) and of Pillow's JPEG at EQUAL bytes, interpolated in log
bytes on their quality 0 .. 100 step 5 curves.
"""
import argparse
import io
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH = 32


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def pillow_curve(frame, fmt, **kw):
    """[(bytes, PSNR)] of Pillow's encoder over quality 0 .. 100 step 5."""
    from PIL import Image
    out = []
    for q in range(0, 101, 5):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(buf, fmt, quality=q, **kw)
        out.append((buf.tell(), psnr(pillow_decode(buf.getvalue()), frame)))
    return sorted(out)


def at_equal_bytes(curve, n):
    """The curve's PSNR at n bytes, interpolated in log bytes; None outside the curve."""
    for (b0, p0), (b1, p1) in zip(curve, curve[1:]):
        if b0 <= n <= b1 and b1 > b0:
            return p0 + (p1 - p0) * (math.log(n) - math.log(b0)) / (math.log(b1) - math.log(b0))
    return None


def rate_distortion():
    import png_encode_ref as P
    import webp_encode_ref as W
    import webp_lossy_encode_ref as R
    edges = np.zeros((64, 96, 3), np.uint8)
    edges[8:40, 10:50] = (255, 255, 255)
    edges[30:60, 40:90] = (20, 200, 240)
    edges[::7, :, 1] = 255
    frames = {"smooth": W.smooth_frame(64, 96), "photo": P.make_frame("photo", 64, 96, seed=7), "edges": edges}
    rows = []
    for name, frame in frames.items():
        webp, jpeg = pillow_curve(frame, "WEBP", method=4), pillow_curve(frame, "JPEG")
        for base_q in (10, 40, 80):
            data, flat = R.encode(frame, base_q), R.encode(frame, base_q, 0)
            ours = psnr(pillow_decode(data), frame)

            def r(v):
                return None if v is None else round(v, 2)
            rows.append(dict(frame=name, base_q=base_q, filter_level=R.default_filter_level(base_q), bytes=len(data), psnr=r(ours),
                             psnr_filter_0=r(psnr(pillow_decode(flat), frame)), pillow_webp_m4_psnr_at_equal_bytes=r(at_equal_bytes(webp, len(data))),
                             pillow_jpeg_psnr_at_equal_bytes=r(at_equal_bytes(jpeg, len(data)))))
    return rows


def measure(encoders, iters):
    import torch
    for enc in encoders.values():
        for _ in range(2):
            enc().files()
    ts, host = {k: [] for k in encoders}, {k: [] for k in encoders}
    for _ in range(iters):
        for k, enc in encoders.items():                                         # alternating: all see the same machine
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = enc()
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
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--rd", action="store_true")
    args = ap.parse_args()
    if args.rd:
        print(json.dumps({"metric": "webp_lossy_encode_rd", "rows": rate_distortion()}))
        return
    import torch
    from maf_yolo_amd import jpeg_encode, webp_encode, webp_lossy, webp_lossy_encode
    from png_encode_probe import picture
    dev = torch.device("cuda:0")
    frames = [torch.from_numpy(picture("photo", i)).to(dev) for i in range(BATCH)]
    if args.once:
        for _ in range(5):
            n = sum(len(f) for f in webp_lossy_encode.encode(frames).files())
        print(json.dumps({"metric": "webp_lossy_encode_probe_once", "files": BATCH, "file_bytes": n}))
        return
    rng = np.random.default_rng(0)
    rects = np.array([(k % BATCH, x, y, x + 64, y + 64) for k, (x, y) in enumerate(zip(rng.integers(0, 640 - 64, 256).tolist(), rng.integers(0, 480 - 64, 256).tolist()))])
    res = {"metric": "webp_lossy_encode_probe", "quality": 75, "iters": args.iters}
    for name, kw in (("frames_32x480x640", {}), ("crops_256x64x64", dict(rects=rects))):
        files = webp_lossy_encode.encode(frames, **kw).files()
        back = webp_lossy.decode(files[:1], device=dev)[0].cpu().numpy()
        if not np.array_equal(back, pillow_decode(files[0])):
            raise SystemExit("Pillow and webp_lossy.decode disagree on a device file")
        encoders = {"webp_lossy": lambda: webp_lossy_encode.encode(frames, **kw), "jpeg": lambda: jpeg_encode.encode(frames, **kw),
                    "webp_lossless": lambda: webp_encode.encode(frames, **kw)}
        res[name] = measure(encoders, args.iters)
        for k, enc in encoders.items():
            res[name][k]["file_bytes"] = sum(len(f) for f in enc().files())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
