"""Cross-check of the VP8 constants: tests/webp_lossy_tables.py and maf-yolo_amd/csrc/vp8_tables.h against each other and against the byte
runs inside a libwebp shared library (its decoder holds the same tables as plain arrays).  Every table of the header is covered: the two
coefficient probability tables, the sub-mode probabilities, the DC and AC quantisers, zigzag, bands and the category bits (cat3 to cat6, which
libwebp keeps as four zero-terminated arrays).

    python tools/vp8_tables_check.py [path to libwebp.so]

Without a path it looks for the system's libwebp.  Prints what it found; exits non-zero on a mismatch.  The proof of the tables is the
fixture set (a wrong entry is a pixel mismatch against Pillow); this is the quick second opinion.
"""
import ctypes.util
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import webp_lossy_tables as T  # noqa: E402


def header_tables():
    with open(os.path.join(ROOT, "maf-yolo_amd", "csrc", "vp8_tables.h")) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    return {name: [int(v) for v in re.findall(r"\d+", body)] for name, body in re.findall(r"(k_vp8_\w+)(?:\[\d+\])+\s*=\s*\{(.*?)\};", text, flags=re.S)}


def library_path(arg):
    if arg:
        return arg
    name = ctypes.util.find_library("webp")
    for d in ("/usr/lib/x86_64-linux-gnu", "/usr/lib64", "/usr/lib", "/usr/local/lib"):
        if name and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise SystemExit("no libwebp found: give its path")


def main():
    h = header_tables()
    pairs = [("coeff_proba0", T.COEFF_PROBA0, np.uint8), ("coeff_update", T.COEFF_UPDATE, np.uint8), ("bmode_proba", T.BMODE_PROBA, np.uint8),
             ("dc_q", T.DC_Q, np.uint8), ("ac_q", T.AC_Q, "<u2"), ("zigzag", np.array(T.ZIGZAG), np.uint8), ("bands", np.array(T.BANDS), np.uint8)]
    bad = 0
    for name, arr, _ in pairs:
        same = h["k_vp8_" + name] == [int(v) for v in np.asarray(arr).reshape(-1)]
        bad += not same
        print("%-14s header == tests: %s" % (name, same))
    same = [v for v in h["k_vp8_cat3456"] if v] == [v for c in T.CAT3456 for v in c]      # the header pads each row with zeros
    bad += not same
    print("%-14s header == tests: %s" % ("cat3456", same))
    path = library_path(sys.argv[1] if len(sys.argv) > 1 else None)
    blob = open(path, "rb").read()
    # libwebp keeps the extra-bit probabilities of the four categories as four zero-terminated arrays of their own
    pairs += [("cat%d" % (3 + i), np.array(c + (0,)), np.uint8) for i, c in enumerate(T.CAT3456)]
    for name, arr, dt in pairs:
        run = np.asarray(arr).reshape(-1).astype(dt).tobytes()
        at = blob.find(run)
        bad += at < 0
        print("%-14s %d bytes %s in %s" % (name, len(run), "at offset %d" % at if at >= 0 else "NOT FOUND", path))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
