"""Writes tests/golden/jpeg_encode_cases.npz with Pillow (libjpeg-turbo, optimize off): small BGR frames, the JPEG file Pillow writes for
each setting, and Pillow's decode of that file as BGR — what the device encoder (maf-yolo_amd/jpeg_encode.py) and the NumPy reference
(tests/jpeg_encode_ref.py) must reproduce byte for byte.

    python tools/make_golden_jpeg_encode.py

Keys: names [n] ("<h>x<w>_<kind>_<420|444>_q<quality>"); meta int32 [n, 4] = h, w, luma sampling factor (2: 4:2:0, 1: 4:4:4), quality;
frame_<h>x<w>_<kind> uint8 [h, w, 3] BGR (shared by the settings); file_<name> uint8; bgr_<name> uint8 [h, w, 3] (Pillow's decode of the
file); large_file / large_meta (480 x 640 smooth frame of jpeg_encode_ref.smooth_frame, quality 95, 4:2:0: only the file is stored).
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_encode_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_encode_cases.npz")
SIZES = [(1, 1), (2, 2), (8, 8), (16, 16), (17, 19), (19, 17), (40, 25), (24, 40), (33, 47)]      # h x w
KINDS = ("random", "ramp", "saturated")
SAMPLINGS = (("4:2:0", 2, "420"), ("4:4:4", 1, "444"))
QUALITIES = (30, 75, 95, 100)


def pillow_file(bgr, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(bgr[..., ::-1]).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def main():
    out, names, meta = {}, [], []
    for si, (h, w) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            frame = R.make_frame(kind, h, w, seed=100 * si + ki)
            out["frame_%dx%d_%s" % (h, w, kind)] = frame
            for ss, hs, tag in SAMPLINGS:
                for q in QUALITIES:
                    name = "%dx%d_%s_%s_q%d" % (h, w, kind, tag, q)
                    data = pillow_file(frame, q, ss)
                    names.append(name)
                    meta.append((h, w, hs, q))
                    out["file_" + name] = np.frombuffer(data, np.uint8)
                    out["bgr_" + name] = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])
    out["names"] = np.array(names)
    out["meta"] = np.array(meta, np.int32)
    out["large_file"] = np.frombuffer(pillow_file(R.smooth_frame(480, 640), 95, "4:2:0"), np.uint8)
    out["large_meta"] = np.array([480, 640, 2, 95], np.int32)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
