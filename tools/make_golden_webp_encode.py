"""Writes tests/golden/webp_encode_cases.npz with the rule book of the lossless WebP encoder (tests/webp_encode_ref.py): small BGR frames, the
targeted frames, and the file the rule book writes for each — what the device encoder (maf-yolo_amd/webp_encode.py) must reproduce byte for byte.

    python tools/make_golden_webp_encode.py

While writing it asserts what the fixture is for: Pillow (libwebp) decodes every file to its frame; all 14 predictor modes are chosen somewhere;
on the photo and smooth frames from 17 x 19 up the file is smaller than png_encode_ref's file of the same frame.

Keys: names [n]; bits int32 [n] (predictor_bits); frame_<name> uint8 [h, w, 3] BGR; file_<name> uint8; targeted [m] and t_bits, t_frame_<name>,
t_file_<name> likewise for webp_encode_ref.targeted_frames(); large_sha256 / large_bytes (the 480 x 640 frame of webp_encode_ref.large_frame,
predictor_bits 4: only the SHA-256 of its file is stored, the frame comes from its seed); pillow_version (the decoder that judged them).
"""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_encode_ref as P  # noqa: E402
import webp_encode_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "webp_encode_cases.npz")


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def main():
    out, modes = {}, set()
    for prefix, key, frames in (("", "names", R.fixture_frames()), ("t_", "targeted", R.targeted_frames())):
        for name, (frame, bits) in frames.items():
            taps = {}
            data = R.encode(frame, bits, taps)
            assert np.array_equal(pillow_decode(data), frame), name
            modes |= set(taps["modes"].tolist())
            if not prefix and name.split("_")[1] in ("photo", "smooth") and frame.shape[0] >= 17:
                assert len(data) < len(P.encode(frame)), "%s: %d bytes, PNG %d" % (name, len(data), len(P.encode(frame)))
            out[prefix + "frame_" + name] = frame
            out[prefix + "file_" + name] = np.frombuffer(data, np.uint8)
        out[key] = np.array(list(frames))
        out["bits" if not prefix else "t_bits"] = np.array([b for _, b in frames.values()], np.int32)
    assert modes == set(range(14)), sorted(modes)
    large = R.encode(R.large_frame())
    assert np.array_equal(pillow_decode(large), R.large_frame())
    out["large_sha256"] = np.array(hashlib.sha256(large).hexdigest())
    out["large_bytes"] = np.array(len(large), np.int64)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print("%s: %d + %d cases, %d bytes" % (OUT, len(out["names"]), len(out["targeted"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
