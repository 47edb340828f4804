"""Writes tests/golden/png_encode_cases.npz with the interpreter's zlib module: small BGR frames and, per filter, the PNG file whose zlib stream
is zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE) over the filtered rows, assembled by the rule book's file layout
(tests/png_encode_ref.py assemble) — what the device encoder (maf-yolo_amd/png_encode.py) and the rule book must reproduce byte for byte.

    python tools/make_golden_png_encode.py

Keys: names [n] ("<h>x<w>_<kind>_<filter>"); meta int32 [n, 3] = h, w, filter type (0 .. 4); frame_<h>x<w>_<kind> uint8 [h, w, 3] BGR (shared
by the filters); file_<name> uint8; zlib_version (the library that wrote them); large_sha256 / large_meta (the 480 x 640 frame of
png_encode_ref.large_frame, filter sub: only the SHA-256 of its file is stored, the frame comes from its seed).
"""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_encode_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "png_encode_cases.npz")
SIZES = [(1, 1), (1, 37), (29, 1), (2, 2), (8, 8), (17, 19), (33, 47), (64, 64)]      # h x w
KINDS = ("noise", "flat", "ramp", "photo", "blocks")
ALL_FILTERS_AT = ((17, 19), (33, 47))                                                  # the other sizes: sub only


def zlib_file(bgr, filt):
    return R.assemble(bgr.shape[1], bgr.shape[0], R.zlib_stream(R.filtered(bgr, filt)))


def main():
    out, names, meta = {}, [], []
    for si, (h, w) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            frame = R.make_frame(kind, h, w, seed=100 * si + ki)
            out["frame_%dx%d_%s" % (h, w, kind)] = frame
            for filt, ft in R.FILTERS.items():
                if filt != "sub" and (h, w) not in ALL_FILTERS_AT:
                    continue
                name = "%dx%d_%s_%s" % (h, w, kind, filt)
                names.append(name)
                meta.append((h, w, ft))
                out["file_" + name] = np.frombuffer(zlib_file(frame, filt), np.uint8)
    out["names"] = np.array(names)
    out["meta"] = np.array(meta, np.int32)
    out["zlib_version"] = np.array(zlib.ZLIB_RUNTIME_VERSION)
    out["large_sha256"] = np.array(hashlib.sha256(zlib_file(R.large_frame(), "sub")).hexdigest())
    out["large_meta"] = np.array([480, 640, 1], np.int32)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
