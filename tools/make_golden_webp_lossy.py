"""Writes tests/golden/webp_lossy_cases.npz: lossy WebP files, Pillow's (libwebp's) pixels of each, libwebp's Y, U and V planes
(WebPDecodeYUV, called through ctypes on this machine's libwebp — here only, never in product code), and malformed files with the status
word the rule book (tests/webp_lossy_ref.py) predicts.

    names, file_<n>, bgr_<n> (Pillow's decode, BGR, alpha dropped), y_<n>, u_<n>, v_<n> (WebPDecodeYUV: w x h and ceil(w / 2) x ceil(h / 2))
    bad_names, badfile_<n>, badstatus_<n>

Before writing it asserts that the rule book equals Pillow AND WebPDecodeYUV on every well-formed case, that Pillow refuses every malformed
one, that every dequantised coefficient of a transcoded case stays within +-2047 (beyond that libwebp's own transforms are not promised to
agree, so no judge exists: no such case is built), and, through the rule book's counters, that the set reaches every path listed in REQUIRED.
Pillow's encoder cannot set most header fields, so transcode() of the rule book writes real image content again with the filter type, level,
sharpness and deltas, the segmentation, the skip probability, the quantiser deltas, the ignored bits and the partition count changed; Pillow
then judges the new file like any other.
"""
import ctypes
import ctypes.util
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import webp_lossy_ref as R  # noqa: E402

REQUIRED = (["ymode%d" % m for m in range(4)] + ["bmode%d" % m for m in range(10)] + ["uvmode%d" % m for m in range(4)] +
            ["tok_eob", "tok0", "tok1", "tok2", "tok3", "tok4", "cat1", "cat2", "cat3", "cat4", "cat5", "cat6", "y2_ac", "skipped",
             "filter_simple", "filter_normal", "filter_none", "inner_on", "inner_off", "hev0", "hev1", "hev2", "type_i4", "type_i16"] +
            ["q%d" % i for i in range(128)])


def pillow_bgr(d):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGBA"))[..., 2::-1])


def pillow_refuses(d):
    try:
        Image.open(io.BytesIO(d)).convert("RGBA").load()
    except Exception:
        return True
    return False


def pillow_file(arr, quality, method, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "WEBP", quality=quality, method=method, **kw)
    return b.getvalue()


_libwebp = None


def libwebp_yuv(d):
    """WebPDecodeYUV of this machine's libwebp -> (Y, U, V) uint8 arrays."""
    global _libwebp
    if _libwebp is None:
        _libwebp = ctypes.CDLL(ctypes.util.find_library("webp") or "libwebp.so.7")
        _libwebp.WebPDecodeYUV.restype = ctypes.c_void_p
        _libwebp.WebPDecodeYUV.argtypes = [ctypes.c_char_p, ctypes.c_size_t] + [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.POINTER(ctypes.c_void_p)] * 2 + \
            [ctypes.POINTER(ctypes.c_int)] * 2
        _libwebp.WebPFree.argtypes = [ctypes.c_void_p]
    w, h, stride, uv_stride = (ctypes.c_int() for _ in range(4))
    u, v = ctypes.c_void_p(), ctypes.c_void_p()
    y = _libwebp.WebPDecodeYUV(d, len(d), w, h, u, v, stride, uv_stride)
    assert y, "WebPDecodeYUV refused the file"

    def plane(p, rows, cols, pitch):
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (rows, pitch))[:, :cols].copy()
    out = (plane(y, h.value, w.value, stride.value), plane(u.value, (h.value + 1) // 2, (w.value + 1) // 2, uv_stride.value),
           plane(v.value, (h.value + 1) // 2, (w.value + 1) // 2, uv_stride.value))
    _libwebp.WebPFree(y)
    return out


def contents(h, w, rng):
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([(x * 5 + y) & 255, (x + y * 3) & 255, (x * y) & 255], -1).astype(np.uint8)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mixed = np.where(((x // 8 + y // 8) & 1)[..., None] == 1, noise, np.stack([x * 3 & 255, y * 2 & 255, (x + y) & 255], -1)).astype(np.uint8)
    flat = np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    return dict(smooth=smooth, noise=noise, mixed=mixed, flat=flat)


def soft(h, w):
    """Low contrast: small coefficient levels, so that a coarse quantiser keeps every coefficient inside +-2047."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([120 + ((x // 4 + y // 3) & 3) * 3, 110 + ((x // 5) & 1) * 4 + y // 8, 130 - x // 6 + ((y // 2) & 1) * 2], -1).astype(np.uint8)


def cut_payload(d, payload):
    return R.replace_payload(d, payload)


def main():
    assert features.check("webp"), "Pillow without libwebp"
    rng = np.random.default_rng(2026)
    good, bad, reached = {}, {}, set()

    def add(name, d, hand_made=False):
        R.counters.clear()
        bgr, planes, st = R.decode_stages(d)
        assert st == 0, name
        want = pillow_bgr(d)
        assert np.array_equal(bgr, want), "%s: the rule book differs from Pillow" % name
        for got, lib_plane, which in zip(planes, libwebp_yuv(d), "YUV"):
            assert np.array_equal(got, lib_plane), "%s: plane %s of the rule book differs from WebPDecodeYUV" % (name, which)
        if hand_made:
            assert R.counters["max_coeff"] <= 2047, "%s: a dequantised coefficient of %d" % (name, R.counters["max_coeff"])
        reached.update(k for k, v in R.counters.items() if v)
        good[name] = (d, want, planes)

    def add_bad(name, d, want_bits):
        _, _, st = R.decode_stages(d)
        assert st == want_bits, "%s: status %d, expected %d" % (name, st, want_bits)
        assert pillow_refuses(d), "%s: Pillow decodes it" % name
        bad[name] = (d, st)

    # ---- written by Pillow
    combos = [(q, m) for q in (1, 30, 75, 90, 100) for m in (0, 4, 6)]
    k = 0
    for w, h in ((1, 1), (2, 3), (15, 15), (16, 16), (17, 17), (17, 33), (33, 17)):
        for kind, arr in contents(h, w, rng).items():
            q, m = combos[k % len(combos)]
            k += 1
            add("%s_%dx%d_q%d_m%d" % (kind, w, h, q, m), pillow_file(arr, q, m))
    big = contents(65, 64, rng)
    add("mixed_64x65_q75_m4", pillow_file(big["mixed"], 75, 4))
    add("noise_64x65_q1_m0", pillow_file(big["noise"], 1, 0))
    add("smooth_64x65_q100_m6", pillow_file(big["smooth"], 100, 6))
    add("noise_64x65_q100_m4", pillow_file(big["noise"], 100, 4))
    big = contents(130, 156, rng)
    add("mixed_156x130_q30_m4", pillow_file(big["mixed"], 30, 4))
    add("smooth_156x130_q90_m6", pillow_file(big["smooth"], 90, 6))
    add("mixed_40x280_q75_m4", pillow_file(contents(280, 40, rng)["mixed"], 75, 4))      # more macroblock rows than a RECON / FILTER band holds
    rgba = np.concatenate([contents(17, 33, rng)["mixed"], rng.integers(0, 256, (17, 33, 1), dtype=np.uint8)], -1)
    d = pillow_file(rgba, 75, 4)
    assert b"VP8X" in d[:32] and b"ALPH" in d, "no VP8X + ALPH file"
    add("rgba_33x17_q75_m4", d)
    exif = Image.Exif()
    exif[0x0112] = 1
    d = pillow_file(contents(20, 24, rng)["smooth"], 75, 4, exif=exif.tobytes(), icc_profile=b"not a real profile, only bytes to skip")
    assert b"VP8X" in d[:32] and b"ICCP" in d and b"EXIF" in d, "no VP8X + ICCP + EXIF file"
    add("iccp_exif_24x20_q75_m4", d)

    # ---- transcoded: header fields Pillow cannot set, over real image content
    base = pillow_file(contents(40, 50, rng)["mixed"], 30, 4)
    f0, _, _ = R.describe(base)
    assert f0.use_segment and f0.update_map, "the base file has no segment map"
    small = pillow_file(contents(17, 17, rng)["mixed"], 30, 4)
    calm = pillow_file(soft(40, 50), 20, 4)
    fc, _, _ = R.describe(calm)
    patch = contents(33, 48, rng)["flat"]
    patch[8:24, 20:40] = rng.integers(0, 256, (16, 20, 3), dtype=np.uint8)          # flat but for one busy patch: the flat macroblocks are skipped
    skipper = pillow_file(patch, 75, 0)                                              # method 0 codes the skip flag
    fs, _, _ = R.describe(skipper)
    assert fs.use_skip and any(mb["skip"] for mb in fs.mbs), "the flat file skips nothing"
    add("skips_48x33_q75_m0", skipper)
    for name, src, ch in (
            ("simple", base, dict(simple=1)), ("simple_level40", base, dict(simple=1, level=40)), ("level0", base, dict(level=0)),
            ("sharp0", base, dict(sharpness=0, level=20)), ("sharp3", base, dict(sharpness=3, level=30)), ("sharp7", base, dict(sharpness=7, level=63)),
            ("hev2", base, dict(level=45)),
            ("lf_deltas", base, dict(use_lf_delta=1, ref_delta=[9, 3, -2, 1], mode_delta=[-12, 2, 0, -1])),
            ("lf_deltas_off_clamp", base, dict(use_lf_delta=1, ref_delta=[-63, 0, 0, 0], mode_delta=[40, 0, 0, 0])),
            ("parts2", base, dict(log2_parts=1)), ("parts4", base, dict(log2_parts=2)), ("parts8", base, dict(log2_parts=3)),
            ("parts8_two_rows", small, dict(log2_parts=3)),
            ("segments_off", base, dict(segmentation="off")), ("segments_absolute", base, dict(segmentation="absolute")),
            ("no_skip_proba", skipper, dict(use_skip=0)),
            ("dq_low_clamp", calm, dict(base_q=3, dq=[-15, -15, -15, -15, -15], segmentation="off")),
            ("dq_high_clamp", calm, dict(base_q=127, dq=[15, 15, 15, 15, 15], segmentation="off")),
            ("dq_mixed", calm, dict(dq=[-15, 15, -8, 15, -15])),
            ("ignored_bits", base, dict(colorspace=1, clamp=1, xscale=2, yscale=3))):
        add("t_" + name, R.transcode(src, **ch), hand_made=True)
    same = R.decode_stages(R.transcode(base))
    assert all(np.array_equal(a, b) for a, b in zip(same[1], R.decode_stages(base)[1])), "transcode without changes changes the planes"
    # every quantiser index: the calm file again with the base index walked through what is still missing
    tiny = pillow_file(soft(16, 16), 20, 4)
    while True:
        missing = [i for i in range(128) if "q%d" % i not in reached]
        if not missing:
            break
        q = min(missing[0], 127)
        add("t_q%d" % q, R.transcode(tiny, base_q=q, dq=[1, 2, 3, 4, 5], segmentation="off" if R.describe(tiny)[0].use_segment else None), hand_made=True)

    lacking = [r for r in REQUIRED if r not in reached]
    assert not lacking, "paths the set does not reach: %s" % lacking

    # ---- malformed
    victim = pillow_file(contents(17, 33, rng)["mixed"], 75, 4)
    fv, st, parts = R.describe(victim)
    assert st == 0 and len(parts) == 2
    s, e = R.vp8_payload(victim)
    payload, want = victim[s:e], pillow_bgr(victim)
    ok_cut = 0
    for c in range(1, 12):
        d = cut_payload(victim, payload[:-c])
        try:
            same = np.array_equal(pillow_bgr(d), want)
        except Exception:
            same = False
        if not same:
            break
        ok_cut = c
    assert ok_cut >= 1, "no byte of the last partition can go"
    add("cut_%d_still_decodes" % ok_cut, cut_payload(victim, payload[:-ok_cut]))             # the flush bytes at the end are never needed
    add_bad("cut_one_more", cut_payload(victim, payload[:-(ok_cut + 1)]), R.STATUS_INPUT_EXHAUSTED)
    tok_begin = parts[1][0] - s
    add_bad("token_partition_half", cut_payload(victim, payload[:tok_begin + (len(payload) - tok_begin) // 2]), R.STATUS_INPUT_EXHAUSTED)
    first = parts[0][1] - parts[0][0]
    half = first // 2
    tag = int.from_bytes(payload[:3], "little") & 31 | half << 5
    d = cut_payload(victim, tag.to_bytes(3, "little") + payload[3:10 + half] + payload[10 + first:])
    st = R.decode_stages(d)[2]
    assert st & R.STATUS_INPUT_EXHAUSTED, "half a first partition decodes"
    add_bad("first_partition_half", d, st)
    two = R.transcode(base, log2_parts=1)
    f2, _, parts2 = R.describe(two)
    s2, e2 = R.vp8_payload(two)
    table = parts2[0][1] - s2
    p2 = bytearray(two[s2:e2])
    p2[table:table + 3] = b"\xff\xff\xff"
    add_bad("partition_size_past_chunk", cut_payload(two, bytes(p2)), R.STATUS_BAD_PARTITIONS)
    eight = R.transcode(small, log2_parts=3)
    _, _, parts8 = R.describe(eight)
    s8, _ = R.vp8_payload(eight)
    add_bad("partition_table_past_chunk", cut_payload(eight, eight[s8:parts8[0][1] + 9]), R.STATUS_BAD_PARTITIONS)     # 21 bytes of sizes are needed

    out = dict(names=np.array(sorted(good)), bad_names=np.array(sorted(bad)))
    for n, (d, bgr, planes) in good.items():
        out["file_" + n] = np.frombuffer(d, np.uint8)
        out["bgr_" + n] = bgr
        out["y_" + n], out["u_" + n], out["v_" + n] = planes
    for n, (d, st) in bad.items():
        out["badfile_" + n] = np.frombuffer(d, np.uint8)
        out["badstatus_" + n] = np.int32(st)
    path = os.path.join(ROOT, "tests", "golden", "webp_lossy_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d malformed, %d bytes" % (path, len(good), len(bad), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
