"""Writes tests/golden/jpeg_orientation_cases.npz with Pillow (libjpeg-turbo): small JPEG files that carry an EXIF orientation (tag 0x0112
in an APP1 segment, written by Pillow's exif=) and, as the expected frame, PIL.ImageOps.exif_transpose of Pillow's decode of the same bytes,
stored BGR: what cv2.imread returns for them.

    python tools/make_golden_jpeg_orientation.py

Keys: names [n]; file_<name> uint8 (the JPEG bytes); bgr_<name> uint8 (the expected frame: [h, w, 3] for orientations 1 to 4, [w, h, 3] for
5 to 8); meta int32 [n, 4] = stored h, stored w, orientation, 1 if progressive (known from how each file was written); tag0_file, tag9_file:
a tag value outside 1 to 8 (refused).  Non-square frames whose sides are no MCU multiples at 4:2:0, 4:4:4 and gray, a one-pixel-wide and a
one-pixel-high frame, and one progressive file per orientation.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_jpeg as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_orientation_cases.npz")


def encode(pixels, orientation, ss, **kw):
    exif = Image.Exif()
    exif[0x0112] = orientation
    return G.encode(pixels, 75, ss, exif=exif, **kw)


def expected(data):
    im = ImageOps.exif_transpose(Image.open(io.BytesIO(data)))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def main():
    cases = []                                                   # (name, bytes, meta)
    gray = lambda h, w: G.gradient(h, w)[..., 0] // 2 + G.gradient(h, w)[..., 2] // 2      # noqa: E731
    for o in range(1, 9):
        for name, pixels, ss, kw in [("s2_13x22", G.gradient(13, 22), 2, {}), ("s0_17x9", G.noise(17, 9, 50 + o), 0, {}),
                                     ("s1_9x14", G.gradient(9, 14), 1, {}), ("gray_5x11", gray(5, 11), 0, {}),
                                     ("s2_7x1", G.gradient(7, 1), 2, {}), ("s0_1x7", G.noise(1, 7, 60 + o), 0, {}),
                                     ("prog_s2_13x22", G.noise(13, 22, 70 + o), 2, dict(progressive=True))]:
            if o == 1 and name not in ("s2_13x22", "prog_s2_13x22"):
                continue                                          # orientation 1 rides along in the mixed calls only
            h, w = pixels.shape[:2]
            cases.append(("o%d_%s" % (o, name), encode(pixels, o, ss, **kw), [h, w, o, int("prog" in name)]))
    out = {"names": np.array([c[0] for c in cases]), "meta": np.array([c[2] for c in cases], np.int32)}
    for name, data, (h, w, o, _) in cases:
        want = expected(data)
        assert want.shape == ((w, h, 3) if o >= 5 else (h, w, 3)), name
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["bgr_" + name] = want
    for o in (0, 9):
        out["tag%d_file" % o] = np.frombuffer(encode(G.gradient(8, 8), o, 0), np.uint8)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
