"""Writes tests/golden/tiff_encode_cases.npz with Pillow / libtiff: small BGR frames and, for each, the strips libtiff wrote at cv2.imwrite's
settings (Compression LZW, Predictor 2, PlanarConfiguration 1, RGB) — what the device encoder (maf-yolo_amd/tiff_encode.py) and the rule book
(tests/tiff_encode_ref.py) must reproduce byte for byte — and, for the BMP encoder (maf-yolo_amd/bmp_encode.py), Pillow's pixel array.

    python tools/make_golden_tiff_encode.py

Keys: names [n] ("<h>x<w>_<kind>"); meta int32 [n, 2] = h, w; frame_<name> uint8 [h, w, 3] BGR; variants [m] ("<name>_r<rows per strip>", the
rows per strip being the cv2 rule's, 1, min(4, h) and h, and "<name>_nopred" without the predictor at the cv2 rule's), and per variant
strips_<variant> uint8 (the strips one behind the other), lens_<variant> int32 (their lengths) and tags_<variant> int32 [11] (TAGS: width,
height, compression, photometric, samples per pixel, rows per strip, planar configuration, predictor or 0, the three BitsPerSample).
large_sha256 / large_lens / large_tags: the 480 x 640 frame of png_encode_ref.large_frame at the cv2 rule's 4 rows per strip (the frame comes
from its seed; of its strips, one behind the other, only the SHA-256 is stored).  bmp_names [k] ("<h>x<w>_<seed>": tiff_encode_ref.make_frame("noise", h, w, seed)) and bmp_<name> uint8: file[54:] as Pillow
writes it.  pillow_version, libtiff_version.
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_encode_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tiff_encode_cases.npz")
SIZES = [(1, 1), (1, 37), (29, 1), (2, 2), (8, 8), (17, 19), (33, 47), (64, 64)]      # h x w
KINDS = ("noise", "flat", "ramp", "photo", "blocks")
TAGS = (256, 257, 259, 262, 277, 278, 284, 317)
BMP_SIZES = [(h, w) for h in (1, 5) for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64)]


def libtiff_file(bgr, rows_per_strip, predictor=True):
    info = {278: int(rows_per_strip)}
    if predictor:
        info[317] = 2
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "TIFF", compression="tiff_lzw", tiffinfo=info)
    return buf.getvalue()


def strips_and_tags(data):
    tags, strips = R.file_strips(data)
    assert tags[273] == sorted(tags[273]) and len(tags[258]) == 3
    return (np.frombuffer(b"".join(strips), np.uint8), np.array([len(s) for s in strips], np.int32),
            np.array([tags.get(t, [0])[0] for t in TAGS] + tags[258], np.int32))


def pillow_bmp(bgr):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "BMP")
    data = buf.getvalue()
    assert data[10:14] == b"\x36\0\0\0"
    return np.frombuffer(data[54:], np.uint8)


def main():
    out, names, meta, variants = {}, [], [], []
    for si, (h, w) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            name = "%dx%d_%s" % (h, w, kind)
            frame = R.make_frame(kind, h, w, seed=100 * si + ki)
            names.append(name)
            meta.append((h, w))
            out["frame_" + name] = frame
            todo = [("%s_r%d" % (name, r), r, True) for r in sorted({R.cv2_rows_per_strip(w, h), 1, min(4, h), h})]
            todo.append((name + "_nopred", R.cv2_rows_per_strip(w, h), False))
            for variant, r, predictor in todo:
                variants.append(variant)
                out["strips_" + variant], out["lens_" + variant], out["tags_" + variant] = strips_and_tags(libtiff_file(frame, r, predictor))
    out["names"], out["meta"], out["variants"] = np.array(names), np.array(meta, np.int32), np.array(variants)
    strips, out["large_lens"], out["large_tags"] = strips_and_tags(libtiff_file(R.large_frame(), R.cv2_rows_per_strip(640, 480)))
    out["large_sha256"] = np.array(hashlib.sha256(strips.tobytes()).hexdigest())
    bmp_names = []
    for i, (h, w) in enumerate(BMP_SIZES):
        name = "%dx%d_%d" % (h, w, 500 + i)
        bmp_names.append(name)
        out["bmp_" + name] = pillow_bmp(R.make_frame("noise", h, w, 500 + i))
    out["bmp_names"] = np.array(bmp_names)
    out["pillow_version"] = np.array(Image.__version__)
    out["libtiff_version"] = np.array(features.version("libtiff"))
    np.savez_compressed(OUT, **out)
    print("%s: %d frames, %d variants, %d BMP cases, %d bytes" % (OUT, len(names), len(variants), len(bmp_names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
