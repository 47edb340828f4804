"""Writes tests/golden/webp_lossy_encode_cases.npz with the rule book of the lossy WebP encoder (tests/webp_lossy_encode_ref.py): small BGR
frames, the arguments, and the file and taps the rule book gives for each — what the device encoder (maf-yolo_amd/webp_lossy_encode.py) must
reproduce byte for byte.

    python tools/make_golden_webp_lossy_encode.py

While writing it asserts, for every case: Pillow (libwebp) decodes the file to exactly webp_lossy_ref.decode_stages' BGR; the unfiltered
planes a decoder reconstructs (webp_lossy_ref.reconstruct(describe(file))) are the reconstruction the encoder predicted from; with
filter_level 0 the decoder's yuv planes are that reconstruction too; the partition count is the one asked for (or what the rows allow).

Keys: names [n]; args int32 [n, 3] (base_q, filter_level or -1 for the default, log2_parts); frame_<name> uint8 [h, w, 3] BGR; file_<name>
uint8; per tap <tap>_<name>: y, u, v (the padded input planes), ry, ru, rv (the unfiltered reconstruction), ymodes, uvmodes, skips, levels
int16 [mb, 25, 16], parts (the partition sizes); pillow_version (the decoder that judged them).
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_encode_ref as P  # noqa: E402
import webp_lossy_encode_ref as E  # noqa: E402
import webp_lossy_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "webp_lossy_encode_cases.npz")
Q = 30                        # the base_q most cases share, so that one call of the device takes them as a batch of mixed sizes


def cases():
    """name -> (frame, base_q, filter_level or None, log2_parts); shapes are h x w."""
    rng = np.random.default_rng(11)
    out = {}
    out["1x1"] = (np.array([[[30, 200, 90]]], np.uint8), Q, None, 3)
    for k, (h, w) in enumerate(((16, 16), (17, 16), (15, 17), (33, 47))):
        out["%dx%d" % (h, w)] = (P.make_frame("photo", h, w, seed=40 + k), Q, None, 3)
    out["33x47_f0"] = (out["33x47"][0], Q, 0, 3)
    flat = P.make_frame("photo", 64, 48, seed=50)
    flat[:, :24] = (130, 130, 130)                           # Y = U = V = 128: nothing to code behind the first column of macroblocks
    out["64x48_flat"] = (flat, Q, None, 3)
    tall = P.make_frame("photo", 130, 70, seed=51)
    for lp in (3, 0, 1, 2):
        out["130x70_p%d" % lp] = (tall, Q, None, lp)
    noise = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    out["48x48_noise_q0"] = (noise, 0, 0, 3)
    out["48x48_noise_q127"] = (noise, 127, None, 3)
    white = np.zeros((32, 32, 3), np.uint8)
    white[:16, :16] = 255
    out["32x32_white_mb"] = (white, 0, 0, 3)                 # the finest Y2 step: the largest Y2 DC level there is for 8-bit samples next to black
    out["32x32_white_mb_f"] = (white, 10, None, 3)
    return out


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def main():
    out, names, args = {}, [], []
    for name, (frame, base_q, level, lp) in cases().items():
        taps = {}
        data = E.encode(frame, base_q, level, lp, taps)
        h, w = frame.shape[:2]
        bgr, yuv, status = R.decode_stages(data)
        assert status == 0 and np.array_equal(pillow_decode(data), bgr), "%s: Pillow and the rule book's decoder disagree" % name
        f, status, parts = R.describe(data)
        assert status == 0 and len(parts) == 1 + (1 << min(lp, ((h + 15) >> 4).bit_length() - 1)), name
        assert [b - a for a, b in parts] == taps["part_sizes"], name
        recon = R.reconstruct(f)
        for got, want in zip(recon, taps["recon"]):
            assert np.array_equal(got, want), "%s: a decoder reconstructs other planes than the encoder predicted from" % name
        if f.level == 0:
            cw, ch = (w + 1) >> 1, (h + 1) >> 1
            for got, want, (hh, ww) in zip(yuv, taps["recon"], ((h, w), (ch, cw), (ch, cw))):
                assert np.array_equal(got, want[:hh, :ww]), name
        names.append(name)
        args.append((base_q, -1 if level is None else level, lp))
        out["frame_" + name] = frame
        out["file_" + name] = np.frombuffer(data, np.uint8)
        for key, plane in zip("yuv", taps["planes"]):
            out["%s_%s" % (key, name)] = plane
        for key, plane in zip(("ry", "ru", "rv"), taps["recon"]):
            out["%s_%s" % (key, name)] = plane
        for key in ("ymodes", "uvmodes", "skips", "levels"):
            out["%s_%s" % (key, name)] = taps[key]
        out["parts_" + name] = np.array(taps["part_sizes"], np.int32)
        print("%-18s %5d bytes, %3d macroblocks, %3d skipped, use_skip %d, luma modes %s, largest |level| %d" % (
            name, len(data), len(f.mbs), int(taps["skips"].sum()), f.use_skip, np.bincount(taps["ymodes"], minlength=4).tolist(), int(np.abs(taps["levels"]).max())))
    out["names"], out["args"] = np.array(names), np.array(args, np.int32)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
