"""Measurements of the PNG decoder (csrc/png_decode.hip, maf-yolo_amd/png.py) on the GPU; prints ONE JSON line and writes it to
profiles/png_probe.json.

    python tools/png_probe.py [--iters N] [--batches 32,256,1024] [--interlaced]

The file is the 480 x 640 picture of tests/golden/jpeg_cases.npz (its large case, decoded by Pillow) re-encoded by Pillow as an RGB PNG and
replicated to B files per call.  Per B:
* images/s of decode(files, check=False) end to end (host parse + staging + copy + the three kernels), wall clock over `iters` calls with
  one synchronisation at the end, and of decode(files) with its status read per call;
* the host's share: wall time of parse + build_blob + fill_blob for the call, and of a call with the device idle behind it (enqueue only);
* per-stage device times from event pairs around maf_png_decode restricted to one stage, and the inflate stage's time per file when every
  file of the call has a wave of its own (B = 32: the per-stream rate, to be read against jpeg_entropy_kernel's per-file time in DESIGN.md);
* bytes moved per call.
The single-thread Pillow decode time of the same file on the same host stands beside them.
--interlaced: instead, the same 480 x 640 pixels assembled by hand (tests/png_ref.py, tests/png_adam7_ref.py: filter types cycled, zlib level 6) as a
plain and as an Adam7 file; per B the per-stage device times of both (decoded with interlaced=True) and of a call that alternates them; one JSON
line, written to profiles/png_probe_interlaced.json.
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
from maf_yolo_amd import lib, png as P  # noqa: E402

DEV = torch.device("cuda:0")


def host_ms(files):
    t0 = time.perf_counter()
    infos = [P.parse(f) for f in files]
    hdr, images, palette = P.build_blob(infos)
    buf = np.empty(int(hdr["total_bytes"]), np.uint8)
    P.fill_blob(buf, hdr, images, palette, files, infos)
    return round((time.perf_counter() - t0) * 1e3, 2)


def stage_times(files, iters, interlaced=False):
    """Event time of each stage alone, on buffers a full decode has filled."""
    infos = [P.parse(f, interlaced) for f in files]
    hdr, images, palette = P.build_blob(infos)
    stage = torch.empty(int(hdr["total_bytes"]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    P.fill_blob(host, hdr, images, palette, files, infos)
    blob = stage.to(DEV)
    inflated = torch.empty(int(hdr["inflated_bytes"]), dtype=torch.uint8, device=DEV)
    rows = torch.empty(int(hdr["rows_bytes"]), dtype=torch.uint8, device=DEV)
    out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=DEV)
    status = torch.empty(len(files), dtype=torch.int32, device=DEV)
    L = lib.load()
    st = torch.cuda.current_stream(DEV)
    res = {}
    for name, mask in (("inflate", P.STAGE_INFLATE), ("unfilter", P.STAGE_UNFILTER), ("convert", P.STAGE_CONVERT), ("all", P.STAGE_ALL)):
        def run():
            lib.check(L.maf_png_decode(host.ctypes.data, blob.data_ptr(), inflated.data_ptr(), rows.data_ptr(), out.data_ptr(), status.data_ptr(),
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
    assert int(status.abs().sum()) == 0
    res["bytes"] = dict(h2d=int(hdr["total_bytes"]), inflated_write_read=2 * int(hdr["inflated_bytes"]), rows_write_read=2 * int(hdr["rows_bytes"]),
                        frames=int(hdr["out_bytes"]))
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
    P.decode(files, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        P.decode(files, device=DEV, check=False)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_async = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(iters):
        P.decode(files, device=DEV)
    t_sync = time.perf_counter() - t0
    c = dict(B=B, img_s_check_false=round(B * iters / t_async, 1), img_s_check_true=round(B * iters / t_sync, 1),
             host_enqueue_ms_per_call=round(t_enq / iters * 1e3, 2), host_parse_staging_ms_per_call=host_ms(files))
    c.update(stage_times(files, max(3, iters)))
    torch.cuda.empty_cache()
    return c


def interlaced_leg(jpg, batches, iters):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import png_adam7_ref as A
    import png_ref as R
    rgb = np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))
    rows = np.ascontiguousarray(rgb).reshape(rgb.shape[0], -1)
    plain = R.encode(rows, rgb.shape[1], 8, 2, level=6)[0]
    laced = A.encode(rows, rgb.shape[1], 8, 2, level=6)[0]
    want = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1]))
    got = P.decode([plain, laced], device=DEV, interlaced=True)
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want)
    res = {"metric": "png_probe_interlaced", "file": "%dx%d RGB 8, filter types cycled, zlib level 6" % rgb.shape[:2],
           "plain_bytes": len(plain), "interlaced_bytes": len(laced), "plain_inflated": P.parse(plain).inflated_size,
           "interlaced_inflated": P.parse(laced, True).inflated_size, "cases": {}}
    for B in batches:
        res["cases"][str(B)] = dict(plain=stage_times([plain] * B, iters, True), interlaced=stage_times([laced] * B, iters, True),
                                    alternating=stage_times([plain, laced] * (B // 2), iters, True))
        torch.cuda.empty_cache()
    return res, "png_probe_interlaced.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--interlaced", action="store_true", help="measure the same pixels as a plain and as an Adam7 file, stage by stage")
    args = ap.parse_args()
    jpg = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["large_file"].tobytes()
    if args.interlaced:
        res, name = interlaced_leg(jpg, [int(b) for b in args.batches.split(",")], max(3, args.iters))
        line = json.dumps(res)
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write(line + "\n")
        print(line)
        return
    buf = io.BytesIO()
    Image.open(io.BytesIO(jpg)).convert("RGB").save(buf, "PNG")
    data = buf.getvalue()
    info = P.parse(data)
    want = torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]))
    assert torch.equal(P.decode([data], device=DEV)[0].cpu(), want)
    res = {"metric": "png_probe", "file": "%dx%d RGB 8, written by Pillow, %d bytes, %d scanline bytes" % (info.height, info.width, len(data), info.inflated_size),
           "pillow_single_thread_ms": pillow_ms(data), "cases": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        res["cases"][str(B)] = measure(data, B, args.iters)
    res["pillow_single_thread_img_s"] = round(1e3 / res["pillow_single_thread_ms"], 1)
    first = res["cases"][args.batches.split(",")[0]]
    res["inflate_ms_per_file_one_wave_each"] = round(first["inflate_us"] / 1e3, 3)      # B <= the chip's free workgroup slots: the time of one stream
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "png_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
