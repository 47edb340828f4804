"""Writes tests/golden/jpeg_cases.npz with Pillow (libjpeg-turbo): synthetic images encoded as baseline JPEG files and the pixels Pillow
decodes from them with libjpeg's defaults (JDCT_ISLOW, fancy upsampling), stored BGR — what cv2.imread returns for the same bytes.

    python tools/make_golden_jpeg.py

Keys: names [n]; file_<name> uint8 (the JPEG bytes); bgr_<name> uint8 [h, w, 3] (expected frame); meta int32 [n, 9] = h, w, components,
Y sampling h, v, restart interval (MCUs), quantisation tables, Huffman tables, 1 if the Huffman tables are optimised — known from how each
file was written, not read back with the parser under test; large_file / large_sha256 (480 x 640, 4:2:0, q 90: the sha256 of the expected
BGR bytes instead of 900 KB of pixels); progressive_file, orientation6_file (the unsupported kinds a header edit cannot make).
"""
import hashlib
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
SIZES = [(1, 1), (7, 9), (8, 8), (17, 33), (48, 64), (75, 100)]          # h x w
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}                             # Pillow's subsampling -> Y sampling factors


def gradient(h, w):
    """A gradient in two channels and an odd-period checker in the third (sharp chroma edges for the fancy upsamplers)."""
    y, x = np.mgrid[0:h, 0:w]
    r = (x * 255 // max(w - 1, 1)).astype(np.uint8)
    g = (y * 255 // max(h - 1, 1)).astype(np.uint8)
    b = ((((x // 3) + (y // 5)) & 1) * 200 + 30).astype(np.uint8)
    return np.stack([r, g, b], -1)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_texture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for c in range(3):
        f = 128 + 70 * np.sin(x / (23.0 + 7 * c) + c) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 3.1 + c)
        f += rng.normal(0, 6 + 6 * c, (h, w)) * (x > w / 2)
        ch.append(np.clip(f, 0, 255))
    return np.stack(ch, -1).astype(np.uint8)


def encode(rgb, quality, ss, **kw):
    buf = io.BytesIO()
    img = Image.fromarray(rgb if rgb.ndim == 3 else rgb, "RGB" if rgb.ndim == 3 else "L")
    if rgb.ndim == 3:
        kw["subsampling"] = ss
    img.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def expected(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def main():
    cases = []          # (name, bytes, meta)

    def add(name, rgb, q, ss, optimize=False, blocks=0, rows=0):
        h, w = rgb.shape[:2]
        kw = {}
        if optimize:
            kw["optimize"] = True
        if blocks:
            kw["restart_marker_blocks"] = blocks
        if rows:
            kw["restart_marker_rows"] = rows
        data = encode(rgb, q, ss, **kw)
        nc = 3 if rgb.ndim == 3 else 1
        hs, vs = SAMPLING[ss] if nc == 3 else (1, 1)
        mcux = -(-w // (8 * hs))
        ri = blocks if blocks else rows * mcux
        cases.append((name, data, [h, w, nc, hs, vs, ri, 2 if nc == 3 else 1, 4 if nc == 3 else 2, int(optimize)]))

    for h, w in SIZES:
        for ss in (0, 1, 2):
            add("grad_q75_%dx%d_s%d" % (h, w, ss), gradient(h, w), 75, ss)
    for i, (h, w) in enumerate([(7, 9), (17, 33), (48, 64), (75, 100)]):
        for ss in (0, 1, 2):
            add("noise_q30_opt_%dx%d_s%d" % (h, w, ss), noise(h, w, 10 + i), 30, ss, optimize=True)
    for i, (h, w) in enumerate([(8, 8), (17, 33), (75, 100)]):
        for ss in (0, 1, 2):
            add("noise_q100_%dx%d_s%d" % (h, w, ss), noise(h, w, 20 + i), 100, ss)
    for ss in (0, 1, 2):
        add("grad_q75_rst2_17x33_s%d" % ss, gradient(17, 33), 75, ss, blocks=2)
    add("noise_q30_opt_rst2_75x100_s2", noise(75, 100, 30), 30, 2, optimize=True, blocks=2)
    for ss in (0, 1, 2):
        add("grad_q75_rstrow_48x64_s%d" % ss, gradient(48, 64), 75, ss, rows=1)
    add("noise_q100_rstrow_75x100_s2", noise(75, 100, 31), 100, 2, rows=1)
    add("gray_q75_17x33", gradient(17, 33)[..., 0] // 2 + gradient(17, 33)[..., 2] // 2, 75, 0)

    out = {"names": np.array([c[0] for c in cases]), "meta": np.array([c[2] for c in cases], np.int32)}
    for name, data, _ in cases:
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["bgr_" + name] = expected(data)
    large = encode(smooth_texture(480, 640, 40), 90, 2)
    out["large_file"] = np.frombuffer(large, np.uint8)
    out["large_sha256"] = np.array(hashlib.sha256(expected(large).tobytes()).hexdigest())
    out["progressive_file"] = np.frombuffer(encode(gradient(16, 16), 75, 2, progressive=True), np.uint8)
    exif = Image.Exif()
    exif[0x0112] = 6
    out["orientation6_file"] = np.frombuffer(encode(gradient(16, 24), 75, 2, exif=exif), np.uint8)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
