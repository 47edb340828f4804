"""Device time of the INTER_AREA launch (csrc/resize_area.hip) beside its INTER_LINEAR sibling maf_augment_resize (csrc/augment.hip) at the
same shapes, in the same run:

    python tools/area_probe.py [--iters 50]

  * 32 x 480 x 640 -> 478 x 638    the reproduce recipe's load (decimation tables, general path)
  * 32 x 1080 x 1920 -> 360 x 640  1080p frames at img_size 640 (exact 3 x 3, integer path)
Each figure is the median over --iters launches of the device time between two events on the launch's stream around the C-ABI call alone
(after 5 warm launches; both kernels' tables are built and uploaded once in front), and (source + destination bytes) / time; the
resize_area_call_us column is the host wall time of one whole resize_area() call (tables, blob copy, launch; not synchronised).
One JSON line per shape."""
import argparse
import importlib
import time
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maf_yolo_amd as M  # noqa: E402
from maf_yolo_amd import lib  # noqa: E402
import letterbox_ref as R  # noqa: E402

LB = importlib.import_module("maf_yolo_amd.letterbox")


def timed(fn, iters, st):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t, out = lib.Timer(), []
    for _ in range(iters):
        t.start(st.cuda_stream)
        fn()
        t.stop(st.cuda_stream)
        torch.cuda.synchronize()
        out.append(t.elapsed_ms() * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    L = lib.load()
    for (h, w), (nh, nw) in [((480, 640), (478, 638)), ((1080, 1920), (360, 640))]:
        B = 32
        frames = [torch.from_numpy(R.synth_frame(h, w, i)).to(dev) for i in range(B)]
        nbytes = B * 3 * (h * w + nh * nw)
        dst = torch.empty(B, nh, nw, 3, dtype=torch.uint8, device=dev)
        ftab, words, _ = LB._area_tables(frames, [(nh, nw)] * B)
        ftab["dst"] += np.uint64(dst.data_ptr())
        host = np.concatenate([ftab.view(np.uint8), words.view(np.uint8)])
        blob = torch.from_numpy(host).to(dev)
        t_host, t_dev = (host.ctypes.data + ftab.nbytes, blob.data_ptr() + ftab.nbytes) if words.size else (None, None)
        area_us, area_min = timed(lambda: lib.check(L.maf_resize_area(host.ctypes.data, blob.data_ptr(), B, t_host, t_dev, words.size, st.cuda_stream)),
                                  a.iters, st)
        assert torch.equal(dst[0], M.resize_area(frames[:1], [(nh, nw)])[0])
        t0 = time.perf_counter()
        for _ in range(10):
            M.resize_area(frames, [(nh, nw)] * B)
        call_us = (time.perf_counter() - t0) / 10 * 1e6
        torch.cuda.synchronize()
        tab = (lib.MafAugmentFrame * B)(*[lib.MafAugmentFrame(f.data_ptr(), f.stride(0), h, w, dst[i].data_ptr(), nh, nw) for i, f in enumerate(frames)])
        tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        lin_us, lin_min = timed(lambda: lib.check(L.maf_augment_resize(C.addressof(tab), tab_dev.data_ptr(), B, st.cuda_stream)), a.iters, st)
        print(json.dumps(dict(shape="%d x %dx%d -> %dx%d" % (B, h, w, nh, nw), path=int(LB.area_plan(h, w, nh, nw)[0]), resize_area_call_us=round(call_us, 1),
                              bytes=nbytes, resize_area_us=round(area_us, 1), resize_area_min_us=round(area_min, 1),
                              resize_area_GBps=round(nbytes / area_us / 1e3, 1), augment_resize_linear_us=round(lin_us, 1),
                              augment_resize_linear_min_us=round(lin_min, 1), augment_resize_linear_GBps=round(nbytes / lin_us / 1e3, 1), iters=a.iters)))


if __name__ == "__main__":
    main()
