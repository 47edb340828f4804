"""Measurements of the TIFF decoder (csrc/tiff_decode.hip, maf-yolo_amd/tiff.py) on the GPU; prints ONE JSON line and writes it to
profiles/tiff_probe.json.

    python tools/tiff_probe.py [--iters N] [--batch 32]

The picture is the 480 x 640 one of tests/golden/jpeg_cases.npz (its large case, decoded by Pillow), written by Pillow as LZW, LZW with
predictor 2, Deflate, PackBits and raw (Pillow's strips: 64 KiB of rows each for the compressed kinds, ONE strip for raw), and once more as LZW
in ONE strip: one wave per strip means such a file decodes on one wave, and the figure puts that limit on record.  Per kind, for B files per call:
* the device time of the two launches of maf_tiff_decode (event pairs, median of `iters`), per batch and per file;
* images/s of decode(files, check=False) end to end (host parse + staging + copy + the launches), one synchronisation at the end;
* the host's share: wall time of parse + build_blob + fill_blob;
* file bytes, strips per file.
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
from PIL import Image, TiffImagePlugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maf_yolo_amd import lib, tiff as T  # noqa: E402

DEV = torch.device("cuda:0")


def host_ms(files):
    t0 = time.perf_counter()
    infos = [T.parse(f) for f in files]
    hdr, images, strips, palette = T.build_blob(infos)
    buf = np.empty(int(hdr["total_bytes"]), np.uint8)
    T.fill_blob(buf, hdr, images, strips, palette, files, infos)
    return round((time.perf_counter() - t0) * 1e3, 2)


def device_us(files, iters):
    """Event time of maf_tiff_decode (both launches) on a blob already on the device."""
    infos = [T.parse(f) for f in files]
    hdr, images, strips, palette = T.build_blob(infos)
    stage = torch.empty(int(hdr["total_bytes"]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    T.fill_blob(host, hdr, images, strips, palette, files, infos)
    blob = stage.to(DEV)
    rows = torch.empty(int(hdr["rows_bytes"]), dtype=torch.uint8, device=DEV)
    out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=DEV)
    status = torch.empty(len(files), dtype=torch.int32, device=DEV)
    L = T._library()
    st = torch.cuda.current_stream(DEV)

    def run():
        lib.check(L.maf_tiff_decode(host.ctypes.data, blob.data_ptr(), rows.data_ptr(), out.data_ptr(), status.data_ptr(), st.cuda_stream))

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    assert int(status.abs().sum()) == 0
    return round(statistics.median(ts), 1), int(hdr["n_strips"]) // len(files), int(hdr["total_bytes"])


def pillow_ms(data):
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def measure(data, B, iters):
    files = [data] * B
    T.decode(files, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        T.decode(files, device=DEV, check=False)
    torch.cuda.synchronize()
    t_async = time.perf_counter() - t0
    us, strips, h2d = device_us(files, max(3, iters))
    torch.cuda.empty_cache()
    return dict(file_bytes=len(data), strips_per_file=strips, device_us_per_batch=us, device_us_per_file=round(us / B, 1),
                img_s_check_false=round(B * iters / t_async, 1), host_parse_staging_ms_per_call=host_ms(files), h2d_bytes=h2d,
                pillow_single_thread_ms=pillow_ms(data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    jpg = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["large_file"].tobytes()
    rgb = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB")))
    want = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1]))
    kinds = {}
    for name, kw in (("lzw", dict(compression="tiff_lzw")), ("lzw_predictor2", dict(compression="tiff_lzw", tiffinfo={317: 2})),
                     ("deflate", dict(compression="tiff_adobe_deflate")), ("packbits", dict(compression="packbits")), ("raw", dict(compression="raw"))):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "TIFF", **kw)
        kinds[name] = buf.getvalue()
    strip_size, TiffImagePlugin.STRIP_SIZE = TiffImagePlugin.STRIP_SIZE, 1 << 24                # Pillow sizes its strips by this
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "TIFF", compression="tiff_lzw")
    TiffImagePlugin.STRIP_SIZE = strip_size
    kinds["lzw_one_strip"] = buf.getvalue()
    res = {"metric": "tiff_probe", "picture": "%dx%d RGB 8" % rgb.shape[:2], "B": args.batch, "cases": {}}
    for name, data in kinds.items():
        info = T.parse(data)
        assert (name != "lzw_predictor2" or info.predictor == 2) and (name != "lzw_one_strip" or len(info.strips) == 1)
        assert torch.equal(T.decode([data], device=DEV)[0].cpu(), want), name
        res["cases"][name] = measure(data, args.batch, args.iters)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "tiff_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
