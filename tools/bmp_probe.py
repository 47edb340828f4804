"""Measurements of the BMP decoder (csrc/bmp_decode.hip, maf-yolo_amd/bmp.py) on the GPU; prints ONE JSON line and writes it to
profiles/bmp_probe.json.

    python tools/bmp_probe.py [--iters N] [--batch 32]

The picture is the 480 x 640 one of tests/golden/jpeg_cases.npz (its large case, decoded by Pillow), written by Pillow as 24-bit, 32-bit, 8-bit
palette and 1-bit BMP, and by the hand encoder of tests/bmp_ref.py (Pillow writes no RLE) as RLE8 (256 colours: mostly absolute runs) and RLE4
(16 colours: longer runs).  One wave per RLE file means such a file is expanded by one wave, and the figure puts that limit on record.  Per
kind, for B files per call:
* the device time of the launches of maf_bmp_decode (event pairs, median of `iters`), per batch and per file;
* images/s of decode(files, check=False) end to end (host parse + staging + copy + the launches), one synchronisation at the end;
* the host's share: wall time of parse + build_blob + fill_blob;
* file bytes.
The single-thread Pillow decode time of the same file on the same host stands beside them.  Every kind is checked against Pillow's pixels first.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmp_ref as R  # noqa: E402
from maf_yolo_amd import bmp as B, lib  # noqa: E402

DEV = torch.device("cuda:0")


def host_ms(files):
    t0 = time.perf_counter()
    infos = [B.parse(f) for f in files]
    hdr, images, rle, palette = B.build_blob(infos)
    buf = np.empty(int(hdr["total_bytes"]), np.uint8)
    B.fill_blob(buf, hdr, images, rle, palette, files, infos)
    return round((time.perf_counter() - t0) * 1e3, 2)


def device_us(files, iters):
    """Event time of maf_bmp_decode (its launches) on a blob already on the device."""
    infos = [B.parse(f) for f in files]
    hdr, images, rle, palette = B.build_blob(infos)
    stage = torch.empty(int(hdr["total_bytes"]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    B.fill_blob(host, hdr, images, rle, palette, files, infos)
    blob = stage.to(DEV)
    planes = torch.empty(max(int(hdr["planes_bytes"]), 16), dtype=torch.uint8, device=DEV)
    out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=DEV)
    status = torch.empty(len(files), dtype=torch.int32, device=DEV)
    L = B._library()
    st = torch.cuda.current_stream(DEV)

    def run():
        lib.check(L.maf_bmp_decode(host.ctypes.data, blob.data_ptr(), planes.data_ptr(), out.data_ptr(), status.data_ptr(), st.cuda_stream))

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    assert int(status.abs().sum()) == 0
    return round(statistics.median(ts), 1), int(hdr["total_bytes"])


def pillow_ms(data):
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def measure(data, batch, iters):
    files = [data] * batch
    B.decode(files, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        B.decode(files, device=DEV, check=False)
    torch.cuda.synchronize()
    t_async = time.perf_counter() - t0
    us, h2d = device_us(files, max(3, iters))
    torch.cuda.empty_cache()
    return dict(file_bytes=len(data), device_us_per_batch=us, device_us_per_file=round(us / batch, 1), img_s_check_false=round(batch * iters / t_async, 1),
                host_parse_staging_ms_per_call=host_ms(files), h2d_bytes=h2d, pillow_single_thread_ms=pillow_ms(data))


def rle_file(img, colors):
    """A palette image of Pillow -> a BI_RLE8 (256 colours) or BI_RLE4 (16) file, bottom-up, by the hand encoder."""
    q = img.quantize(colors, dither=Image.Dither.NONE)
    pal = np.array(q.getpalette()[:3 * colors], np.uint8).reshape(colors, 3)[:, ::-1]
    plane = np.asarray(q)[::-1]
    rle4 = colors == 16
    return R.rle_file(plane.shape[1], plane.shape[0], R.rle_records(plane, rle4), rle4, pal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    jpg = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["large_file"].tobytes()
    img = Image.open(io.BytesIO(jpg)).convert("RGB")
    kinds = {}
    for name, mode in (("bgr24", "RGB"), ("bgra32", "RGBA"), ("palette8", "P"), ("bilevel1", "1")):
        buf = io.BytesIO()
        img.convert(mode).save(buf, "BMP")
        kinds[name] = buf.getvalue()
    kinds["rle8_256_colours"] = rle_file(img, 256)
    kinds["rle4_16_colours"] = rle_file(img, 16)
    res = {"metric": "bmp_probe", "picture": "%dx%d" % (img.size[1], img.size[0]), "B": args.batch, "cases": {}}
    for name, data in kinds.items():
        want = torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]))
        assert torch.equal(B.decode([data], device=DEV)[0].cpu(), want), name
        res["cases"][name] = measure(data, args.batch, args.iters)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "bmp_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
