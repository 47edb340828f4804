"""Writes tests/golden/webp_cases.npz: lossless WebP files, Pillow's (libwebp's) pixels of each, the rule book's argb tap, and malformed files with
the status word the rule book predicts.

    names, file_<n>, bgr_<n> (Pillow's decode, BGR, alpha dropped), argb_<n> (tests/webp_ref.py: the main image before the inverse transforms)
    bad_names, badfile_<n>, badstatus_<n>

Before writing it asserts that the rule book equals Pillow on every well-formed case, that Pillow refuses every malformed one (one that it
accepts is dropped) and, through the rule book's counters, that the set reaches every path listed in REQUIRED.  Pillow-written files come from a
pool of contents x methods x qualities; a file is kept only when it reaches a path no kept file has reached, so the set stays small.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import webp_ref as R  # noqa: E402

REQUIRED = (["pred_mode_%d" % m for m in range(16)] + ["order_" + o for o in ("", "3", "0", "1", "2", "20", "01", "201", "30")] +
            ["pack_8", "pack_4", "pack_2", "pack_1", "index_past_palette", "cache_bits_1", "cache_bits_11", "meta_groups_many",
             "simple1_1bit", "simple1_8bit", "simple2_1bit", "simple2_8bit", "normal_max_symbol", "normal_plain", "token16", "token17", "token18",
             "token16_first", "plane_code", "far_distance", "plane_clamp", "copy_distance_1", "copy_overlap", "copy_across_row", "copy_4096",
             "copy_beyond_8192", "cache_hit"])


def pillow_bgr(d):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGBA"))[..., 2::-1])


def pillow_file(arr, mode, palette=None, **kw):
    im = Image.fromarray(arr, mode)
    if palette is not None:
        im.putpalette([int(v) for v in palette.reshape(-1)])
    b = io.BytesIO()
    im.save(b, "WEBP", lossless=True, **kw)
    return b.getvalue()


def contents(h, w, rng):
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([(x * 3 + y) & 255, (x + y * 2) & 255, (x * y) & 255], -1).astype(np.uint8)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mix = np.where(((x // 8 + y // 8) & 1)[..., None] == 1, smooth, noise).astype(np.uint8)
    flat = np.stack([(x // 5) * 9 & 255, (y // 3) * 7 & 255, ((x // 7 + y // 4) & 3) * 60], -1).astype(np.uint8)
    return dict(smooth=smooth, noise=noise, mix=mix, flat=flat)


def run(d):
    """One decode of the rule book -> (bgr, argb, status, the counters it touched)."""
    R.COUNTERS.clear()
    bgr, argb, st = R.decode_stages(d)
    return bgr, argb, st, set(R.COUNTERS)


def main():
    assert features.check("webp"), "Pillow without libwebp"
    rng = np.random.default_rng(2026)
    good, reached = {}, set()

    def keep(name, d, force=True):
        bgr, argb, st, keys = run(d)
        want = pillow_bgr(d)
        assert st == 0 and np.array_equal(bgr, want), name
        if not force and not (keys & set(REQUIRED)) - reached:
            return
        reached.update(keys)
        good[name] = (d, want, argb)

    # the sizes, Pillow-written
    for h, w in ((1, 1), (9, 1), (1, 9), (33, 17), (65, 64), (130, 156)):
        c = contents(h, w, rng)
        keep("mix_m4_%dx%d" % (w, h), pillow_file(c["mix"], "RGB", method=4))
    c = contents(33, 17, rng)
    keep("rgba_m4_17x33", pillow_file(np.concatenate([c["smooth"], c["noise"][..., :1]], -1), "RGBA", method=4, exact=True))
    # palettes at 19 wide: 8 / 4 / 2 / 2 / 1 pixels per packed pixel
    for n in (2, 3, 5, 17, 200):
        idx = rng.integers(0, n, (7, 19)).astype(np.uint8)
        keep("pal%d_19x7" % n, pillow_file(idx, "P", palette=rng.integers(0, 256, (n, 3)), method=4))
    # the pool: kept where a file reaches something new
    for h, w in ((33, 17), (40, 50), (65, 64)):
        c = contents(h, w, rng)
        for kind, arr in c.items():
            for m in (0, 4, 6):
                for q in (20, 75, 100):
                    keep("%s_m%d_q%d_%dx%d" % (kind, m, q, w, h), pillow_file(arr, "RGB", method=m, quality=q), force=False)
    # a VP8X file with ICCP and an odd-sized unknown chunk in front of VP8L
    pay = R.walk(good["mix_m4_17x33"][0])[0]
    keep("vp8x_iccp_odd_17x33", R.riff(pay, extended=(17, 33, 0x20), before=((b"ICCP", bytes(range(33))), (b"ABCD", b"xyz"))))

    # by hand
    def key_of(v, bits):
        return (R.HASH * v & 0xffffffff) >> (32 - bits)

    def lits(n, step=0x030507):
        return [("lit", 0xff000000 | (i * step & 0xffffff)) for i in range(n)]

    keep("hand_pred_14_15_9x9", R.riff(R.hand_payload(9, 9, [("pred", 2, [(14 + (i & 1)) << 8 | 0xff000000 for i in range(9)])])))
    keep("hand_pred_all_modes_33x17", R.riff(R.hand_payload(33, 17, [("pred", 2, [(i % 16) << 8 | 0xff000000 for i in range(9 * 5)])])))
    keep("hand_cross_alone_9x5", R.riff(R.hand_payload(9, 5, [("cross", 2, [0xff000000 | (37 * i + 200 & 255) << 16 | (91 * i + 7 & 255) << 8 | (53 * i + 130 & 255) for i in range(6)])])))
    keep("hand_green_alone_9x5", R.riff(R.hand_payload(9, 5, [("green",)])))
    pal3 = [0xff102030, 0x00f0e0d0, 0x01010101]
    keep("hand_palette_alone_past_19x5", R.riff(R.hand_payload(19, 5, [("palette", pal3)])))
    keep("hand_palette_then_pred_19x5", R.riff(R.hand_payload(19, 5, [("palette", pal3), ("pred", 2, [(m << 8) | 0xff000000 for m in (11, 12, 13, 5)])])))
    keep("hand_all_four_19x6", R.riff(R.hand_payload(19, 6, [("cross", 2, [0xff112233 + i for i in range(10)]), ("palette", pal3 + [0x7f000000]), ("green",),
                                                             ("pred", 2, [(m << 8) | 0xff000000 for m in (1, 2, 3, 4)])])))
    for bits in (1, 11):
        a, b = 0xff123456, 0x80fedcba
        ops = [("lit", a), ("lit", b), ("cache", key_of(a, bits)), ("cache", key_of(b, bits)), ("copy", 3, 121 + 1), ("cache", key_of(a, bits))] + lits(5)
        ops += [("cache", key_of(ops[-1][1], bits))]
        keep("hand_cache%d_4x3" % bits, R.riff(R.hand_payload(4, 3, ops=ops, cache_bits=bits)))
    clamp_dc = R.K.index(0x1f) + 1
    keep("hand_plane_clamp_5x4", R.riff(R.hand_payload(5, 4, ops=lits(3) + [("copy", 7, clamp_dc)] + lits(4) + [("copy", 6, R.K.index(0x18) + 1)])))
    keep("hand_copy_4096_70x60", R.riff(R.hand_payload(70, 60, ops=lits(4) + [("copy", 4096, 120 + 3)] + lits(30) + [("copy", 70, 120 + 100)])))
    # 100 literals, rows copied down to pixel 9000, then copies that reach back further than 8192 pixels (one of them with a colour cache
    # whose slots several pixels of one copy share)
    far = lits(100) + [("copy", 4096, 120 + 100), ("copy", 4096, 120 + 100), ("copy", 708, 120 + 100), ("copy", 900, 120 + 8950), ("copy", 100, 120 + 9899)]
    keep("hand_far_copies_100x100", R.riff(R.hand_payload(100, 100, ops=far)))
    keep("hand_far_copies_cache3_100x100", R.riff(R.hand_payload(100, 100, ops=far[:-1] + [("cache", key_of(far[5][1], 3))] + lits(99, 0x010203), cache_bits=3)))
    keep("hand_simple_codes_6x2", R.riff(R.hand_payload(6, 2, ops=[("lit", 0xff000100 if i % 3 else 0xff000000) for i in range(12)], code_style="simple")))
    keep("hand_meta_3_groups_9x9", R.riff(R.hand_payload(9, 9, ops=lits(81), meta=(2, [0xff000000 | (i % 3) << 8 for i in range(9)]))))
    flat8 = lambda bw: R.put_normal(bw, [8] * 256, tokens=[(8, 0)] * 256)      # noqa: E731  a code-length code of one literal: tokens of no bits
    keep("hand_zero_bit_tokens_8x8", R.riff(R.hand_payload(8, 8, ops=lits(64, 0x010101), override={1: flat8})))

    missing = [k for k in REQUIRED if k not in reached]
    assert not missing, missing

    # malformed: one cause each
    bad = {}

    def keep_bad(name, d, want):
        st = run(d)[2]
        assert st == want, (name, st, want)
        try:
            Image.open(io.BytesIO(d)).convert("RGBA").load()
        except Exception:
            bad[name] = (d, st)
            return
        print("dropped (Pillow accepts it):", name)

    pay = R.walk(good["mix_m4_64x65"][0])[0]
    keep_bad("stream_cut_to_half", R.riff(pay[:len(pay) // 2]), R.ST_INPUT_EXHAUSTED)
    ops9 = [("lit", 0xff000000 | i) for i in range(9)]                # red 0: a symbol of every overridden red code below
    keep_bad("oversubscribed_code", R.riff(R.hand_payload(3, 3, ops=ops9, override={1: lambda bw: R.put_normal(bw, [1, 1, 1] + [0] * 253)})), R.ST_BAD_CODE_LENGTHS)
    keep_bad("incomplete_code", R.riff(R.hand_payload(3, 3, ops=ops9, override={1: lambda bw: R.put_normal(bw, [1, 2] + [0] * 254)})), R.ST_BAD_CODE_LENGTHS)
    keep_bad("max_symbol_above_alphabet", R.riff(R.hand_payload(3, 3, ops=ops9, override={4: lambda bw: R.put_normal(bw, [1, 1] + [0] * 38, max_symbol=256)})),
             R.ST_BAD_CODE_LENGTHS)
    keep_bad("zero_run_past_alphabet", R.riff(R.hand_payload(3, 3, ops=ops9, override={4: lambda bw: R.put_normal(bw, [1, 1] + [0] * 38, tokens=[(1, 0), (1, 0), (18, 127)])})),
             R.ST_BAD_CODE_LENGTHS)
    keep_bad("cache_bits_0", R.riff(R.hand_payload(3, 3, ops=ops9, cache_bits=0)), R.ST_BAD_CACHE_BITS)
    keep_bad("cache_bits_12", R.riff(R.hand_payload(3, 3, ops=ops9, cache_bits=12)), R.ST_BAD_CACHE_BITS)
    keep_bad("transform_twice", R.riff(R.hand_payload(3, 3, [("green",), ("green",)], ops=ops9)), R.ST_BAD_TRANSFORM)
    keep_bad("distance_beyond_produced", R.riff(R.hand_payload(3, 3, ops=lits(1) + [("copy", 1, 122)] + lits(7))), R.ST_DISTANCE_TOO_FAR)
    keep_bad("copy_past_last_pixel", R.riff(R.hand_payload(3, 3, ops=lits(1) + [("copy", 16, 121)])), R.ST_COPY_PAST_END)
    assert len(bad) >= 8, sorted(bad)

    out = {"names": np.array(list(good)), "bad_names": np.array(list(bad))}
    for n, (d, bgr, argb) in good.items():
        out["file_" + n] = np.frombuffer(d, np.uint8)
        out["bgr_" + n] = bgr
        out["argb_" + n] = argb
    for n, (d, st) in bad.items():
        out["badfile_" + n] = np.frombuffer(d, np.uint8)
        out["badstatus_" + n] = np.int32(st)
    path = os.path.join(ROOT, "tests", "golden", "webp_cases.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print("%d cases, %d malformed, %d bytes -> %s" % (len(good), len(bad), size, path))
    print("kept:", ", ".join(good))


if __name__ == "__main__":
    main()
