"""The rule book of the lossless WebP encoder (csrc/webp_encode.hip, maf-yolo_amd/webp_encode.py) in NumPy: the "profile" of VP8L it writes.
Its judges are decoders: libwebp through Pillow, and tests/webp_ref.py decode_stages (tests/test_webp_encode_host.py).  libwebp's ENCODER is no
judge: its bytes follow heuristics no specification fixes.

Every rule:
* container: RIFF size WEBP, ONE VP8L chunk, a zero pad byte behind an odd payload; no VP8X, no metadata.  The payload begins 0x2f, w - 1 and
  h - 1 in 14 bits each, alpha hint 0, version 0.  A side is at most 16384;
* transforms, in stream order: subtract-green, then the predictor transform with `predictor_bits` (2 .. 9, default 4).  No cross-colour
  transform, no colour indexing.  The encoder subtracts green first (red and blue lose green modulo 256) and predicts on that picture;
  alpha is 255 everywhere, so its residual is 0 everywhere;
* the mode of a block of 2^bits x 2^bits pixels: the cost of mode m is the sum, over the block's pixels with x >= 1 and y >= 1 (the others
  do not depend on the mode) and the R, G, B channels, of min(v, 256 - v) of the residual byte v under m; the lowest cost wins, a tie goes to
  the lowest mode.  Whatever the mode, row 0 predicts from L, column 0 from T, pixel (0, 0) from 0xff000000; the TR of the last column is the
  first pixel of the current row (the next word in memory), as in the decoder.  Prediction reads the un-predicted picture;
* tokens: copies at distance 1 only (distance code 2: dx 1, dy 0), from the run rule.  A maximal run of R equal pixels of an image (runs
  cross rows) gives one literal, then with r = R - 1: r // 4096 copies of 4096, then one copy of r % 4096 when that is >= 3, else that many
  literals.  A token here is a uint32: 0x80000000 | length for a copy, else the literal's R, G, B bytes (pixel & 0xffffff; the alpha byte is
  the same in every pixel of an image).  No colour cache, no entropy image: one group of five codes per image;
* the five codes of an image (green + length: 280 symbols; red, blue, alpha: 256; distance: 40), from the token counts; a code nothing uses
  counts symbol 0 once.  The distance symbol of distance code 2 is 1; a length L has the prefix symbol 256 + prefix_encode(L);
    - one or two used symbols, all below 256: a SIMPLE code (1, count - 1, is_first_8bits = first symbol > 1, the symbols in rising order).
      One symbol is read with zero bits, two symbols take the codes 0 and 1 in rising order;
    - otherwise a NORMAL code whose lengths are zlib's build_tree / gen_bitlen (png_encode_ref.build_tree: the heap filled in symbol order,
      the lower frequency first and on a tie the lower depth, the overflow repair) limited to 15 bits, canonical codes (gen_codes).  A single
      used symbol >= 256 cannot happen: every image starts with a literal, and the distance alphabet is below 256;
    - a normal code's description: 0; the lengths of ALL symbols of the alphabet (no max_symbol: the bit is 0) as the tokens zlib's scan_tree
      gives (png_encode_ref._walk_tree: 16 repeats 3 .. 6, 17 zeros 3 .. 10, 18 zeros 11 .. 138; the greedy rule with its 138/3, 6/3, 7/4
      limits — every 16 it writes follows the length it repeats, so VP8L's "last non-zero length" is that length); the code-length code is
      build_tree over the tokens' counts limited to 7 bits (fewer than two used tokens: zlib forces a second one), sent as 4 + 4 bits counts
      of 3-bit lengths in VP8L's order 17, 18, 0, 1, ..., cut behind the last non-zero one but no shorter than 4;
* the predictor sub-image, ceil(w / 2^bits) x ceil(h / 2^bits) pixels 0xff000000 | mode << 8, is an entropy-coded image like the main one
  and goes through the same tokeniser, codes and bits, without the entropy-image bit.
encode() -> the file, and through `taps`: argb, modes, and per image (sub-image, main) px, tokens, hist, lengths, codes, head_bits, bitoff; payload.
"""
import numpy as np

import png_encode_ref as P
import webp_ref as R

MAX_COPY = 4096
MAX_SIDE = 16384
ALPHABETS = (280, 256, 256, 256, 40)
COPY = 0x80000000
LEAD_BITS = 50
_ZEROS = [0] * 280


# ---------------------------------------------------------------- transforms

def gather(bgr):
    """uint8 [h, w, 3] BGR -> uint32 [h * w] ARGB with green subtracted."""
    f = bgr.astype(np.uint32).reshape(-1, 3)
    b, g, r = f[:, 0], f[:, 1], f[:, 2]
    return (np.uint32(0xff000000) | (((r - g) & 255) << 16) | (g << 8) | ((b - g) & 255)).astype(np.uint32)


def ungather(argb, h, w):
    """The inverse of gather -> uint8 [h, w, 3] BGR."""
    a = np.asarray(argb, np.uint32)
    g = a >> 8 & 255
    return np.stack([(a & 255) + g & 255, g, (a >> 16 & 255) + g & 255], -1).astype(np.uint8).reshape(h, w, 3)


def _channels(a):
    return np.stack([a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255], -1).astype(np.int64)


def _pack(c):
    c = c.astype(np.uint32)
    return c[..., 0] << 24 | c[..., 1] << 16 | c[..., 2] << 8 | c[..., 3]


def predictions(argb, w, h):
    """-> int64 [14, h * w, 4]: the prediction of every mode at every pixel, A, R, G, B (webp_ref.predict, vectorised), the border rules applied."""
    n = w * h
    c = _channels(argb)
    p = np.arange(n)
    black = np.array([255, 0, 0, 0], np.int64)

    def at(off):
        return c[np.clip(p + off, 0, n - 1)]
    L, T, TL, TR = at(-1), at(-w), at(-w - 1), at(-w + 1)
    avg = lambda a, b: (a + b) >> 1
    sel = np.abs(T - TL).sum(-1) < np.abs(L - TL).sum(-1)
    A = avg(L, T)
    d = A - TL
    half = np.where(d < 0, -((-d) >> 1), d >> 1)
    out = np.stack([np.broadcast_to(black, c.shape), L, T, TR, TL, avg(avg(L, TR), T), avg(L, TL), avg(L, T), avg(TL, T), avg(T, TR),
                    avg(avg(L, TL), avg(T, TR)), np.where(sel[:, None], L, T), np.clip(L + T - TL, 0, 255), np.clip(A + half, 0, 255)])
    y, x = p // w, p % w
    out[:, y == 0] = L[y == 0]
    out[:, x == 0] = T[x == 0]
    out[:, 0] = black
    return out


def choose_modes(argb, w, h, bits):
    """-> (modes int64 [bh * bw], residual pixels uint32 [h * w])."""
    n = w * h
    pred = predictions(argb, w, h)
    res = (_channels(argb)[None] - pred) & 255
    v = res[:, :, 1:]
    cost = np.minimum(v, 256 - v).sum(-1)
    p = np.arange(n)
    y, x = p // w, p % w
    bw, bh = R.subsample(w, bits), R.subsample(h, bits)
    blk = (y >> bits) * bw + (x >> bits)
    inner = (x >= 1) & (y >= 1)
    total = np.zeros((14, bw * bh), np.int64)
    for m in range(14):
        total[m] = np.bincount(blk[inner], cost[m][inner], minlength=bw * bh).astype(np.int64)
    modes = total.argmin(0)                                  # the first of equal minima: the lowest mode
    return modes, _pack(res[modes[blk], p])


# ---------------------------------------------------------------- tokens and codes

def tokenise(px):
    """The run rule -> uint32 tokens."""
    px = np.asarray(px, np.uint32)
    start = np.flatnonzero(np.concatenate([[True], px[1:] != px[:-1]]))
    run_len = np.diff(np.concatenate([start, [px.size]]))
    q, rem = np.divmod(run_len - 1, MAX_COPY)
    ntok = 1 + q + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(run_len.size), ntok)
    k = np.arange(int(ntok.sum())) - np.repeat(np.cumsum(ntok) - ntok, ntok)
    lit = px[start][run] & 0xffffff
    return np.where(k == 0, lit, np.where(k <= q[run], COPY | MAX_COPY, np.where(rem[run] >= 3, COPY | rem[run], lit))).astype(np.uint32)


def _prefix(lengths):
    """Copy lengths (>= 3; smaller values are mapped as 3) -> (prefix symbol, extra bits, their count), webp_ref.prefix_encode vectorised."""
    d = np.maximum(np.asarray(lengths, np.int64), 3) - 1
    hb = np.floor(np.log2(np.maximum(d, 1))).astype(np.int64)
    hb = np.where((1 << hb) > d, hb - 1, np.where((2 << hb) <= d, hb + 1, hb))
    e = hb - 1
    small = d < 4
    return np.where(small, d, 2 * hb + (d >> np.maximum(e, 0) & 1)), np.where(small, 0, d & ((1 << np.maximum(e, 0)) - 1)), np.where(small, 0, e)


def histograms(tokens, alpha):
    tokens = np.asarray(tokens, np.int64)
    copy = tokens >= COPY
    lit = tokens[~copy]
    sym = _prefix(tokens[copy] & 0xffff)[0]
    h = [np.bincount(np.concatenate([lit >> 8 & 255, 256 + sym]), minlength=280), np.bincount(lit >> 16 & 255, minlength=256),
         np.bincount(lit & 255, minlength=256), np.zeros(256, np.int64), np.zeros(40, np.int64)]
    h[3][alpha] = lit.size
    h[4][1] = int(copy.sum())
    return [x.astype(np.int64) for x in h]


def build_code(freq, alphabet, stats=None):
    """-> (lengths [alphabet] (0 for the one symbol of a one-symbol code), bit-reversed codes, the description's fields [(value, bits)])."""
    used = [int(s) for s in np.flatnonzero(freq)] or [0]
    lengths = [0] * alphabet
    if len(used) <= 2 and used[-1] < 256:
        first8 = int(used[0] > 1)
        fields = [(1, 1), (len(used) - 1, 1), (first8, 1), (used[0], 8 if first8 else 1)]
        codes = [0] * alphabet
        if len(used) == 2:
            fields.append((used[1], 8))
            lengths[used[0]] = lengths[used[1]] = 1
            codes[used[1]] = 1
        return lengths, codes, fields
    assert len(used) >= 2, "a single used symbol above 255 cannot happen"
    st = P._State()
    lengths, _ = P.build_tree([int(v) for v in freq], alphabet, None, _ZEROS, 0, 15, st)
    codes = P.gen_codes(lengths, alphabet - 1)
    toks = []
    P._walk_tree(lengths, alphabet - 1, lambda s, c: toks.append((s, c)))
    blfreq = [0] * 19
    for s, _ in toks:
        blfreq[s] += 1
    bllen, _ = P.build_tree(blfreq, 19, None, _ZEROS, 0, 7, st)
    blcode = P.gen_codes(bllen, 18)
    if stats is not None:
        stats.append(tuple(st.overflow))
    n = max(4, max(i for i, s in enumerate(R.CL_ORDER) if bllen[s]) + 1)
    fields = [(0, 1), (n - 4, 4)] + [(bllen[R.CL_ORDER[i]], 3) for i in range(n)] + [(0, 1)]
    for s, c in toks:
        fields.append((blcode[s], bllen[s]))
        if c is not None:
            fields.append((c - (3, 3, 11)[s - 16], (2, 3, 7)[s - 16]))
    return lengths, codes, fields


def image_bits(px, alpha, taps=None, stats=None):
    """An entropy-coded image's bits from its five codes on (what follows the cache bit and, in the main image, the entropy-image bit)."""
    tokens = tokenise(px)
    hist = histograms(tokens, alpha)
    built = [build_code(f, a, stats) for f, a in zip(hist, ALPHABETS)]
    heads = [P._bits_of([v for v, _ in fl], [b for _, b in fl]) for _, _, fl in built]
    L = [np.array(b[0], np.int64) for b in built]
    C = [np.array(b[1], np.int64) for b in built]
    t = tokens.astype(np.int64)
    copy = t >= COPY
    sym, xv, xb = _prefix(t & 0xffff)
    g = np.where(copy, 256 + sym, t >> 8 & 255)
    r, b = t >> 16 & 255, t & 255
    z = np.zeros(t.size, np.int64)
    vals = np.stack([C[0][g], np.where(copy, xv, C[1][r]), np.where(copy, C[4][1], C[2][b]), np.where(copy, z, C[3][alpha])], 1)
    nbits = np.stack([L[0][g], np.where(copy, xb, L[1][r]), np.where(copy, L[4][1], L[2][b]), np.where(copy, z, L[3][alpha])], 1)
    body = P._bits_of(vals.reshape(-1), nbits.reshape(-1))
    if taps is not None:
        taps.update(px=np.asarray(px, np.uint32), tokens=tokens, hist=hist, lengths=L, codes=C, head_bits=[h.size for h in heads], data_bits=body.size)
    return np.concatenate(heads + [body])


def encode(frame, predictor_bits=4, taps=None, stats=None):
    """uint8 [h, w, 3] BGR -> the WebP file (bytes)."""
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    assert 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and 2 <= predictor_bits <= 9
    argb = gather(frame)
    modes, res = choose_modes(argb, w, h, predictor_bits)
    sub = (np.uint32(0xff000000) | (modes.astype(np.uint32) << 8)).astype(np.uint32)
    t_sub, t_main = {}, {}
    lead = P._bits_of([0x2f, w - 1, h - 1, 0, 0, 1, 2, 1, 0, predictor_bits - 2, 0], [8, 14, 14, 1, 3, 1, 2, 1, 2, 3, 1])
    assert lead.size == LEAD_BITS
    b_sub = image_bits(sub, 255, t_sub, stats)
    b_main = image_bits(res, 0, t_main, stats)
    bits = np.concatenate([lead, b_sub, np.zeros(3, np.uint8), b_main])
    payload = np.packbits(bits, bitorder="little").tobytes()
    if taps is not None:
        t_sub["bitoff"], t_main["bitoff"] = LEAD_BITS, LEAD_BITS + b_sub.size + 3
        taps.update(argb=argb, modes=modes, images=[t_sub, t_main], payload=payload)
    return R.riff(payload)


# ---------------------------------------------------------------- frames the fixtures and the tests share

def one_row(residuals):
    """The BGR frame [1, n, 3] whose residual pixels (row 0 predicts from L, pixel 0 from black) are `residuals` (uint32, alpha byte ignored)."""
    c = _channels(np.asarray(residuals, np.uint32))
    c[:, 0] = 0
    px = np.cumsum(c, 0) & 255
    px[:, 0] = 255
    return ungather(_pack(px), 1, len(residuals))


def one_column(residuals):
    """Likewise [n, 1, 3]: column 0 predicts from T."""
    return np.ascontiguousarray(one_row(residuals).transpose(1, 0, 2))


def runs_of(remainders, filler=0x010203):
    """Residuals with one run of r + 1 equal pixels per entry, the runs kept apart by two pixels that differ from their neighbours."""
    out = []
    for i, r in enumerate(remainders):
        out += [0x050607 + i] * (r + 1) + [filler, filler + 0x010101]
    return np.array(out, np.uint32)


def green_counts(counts):
    """{green value: count} -> a one-row frame whose residuals are those greens (no two equal neighbours), red and blue 0."""
    return one_row(P.spread(counts).astype(np.uint32) << 8)


def fibonacci_counts(terms):
    """Green counts 1, 1, 2, 3, 5, ...: a Huffman tree that is a chain `terms` - 1 deep (17 terms are 4180 pixels)."""
    f = [1, 1]
    while len(f) < terms:
        f.append(f[-1] + f[-2])
    return {10 + i: c for i, c in enumerate(f)}


def synth(w, h, bits, block_modes, seed, keep=5):
    """A frame built the way the decoder rebuilds one: block by block the pixel IS the prediction of the block's assigned mode, except that
    every `keep`-th pixel or so, row 0 and column 0 are random — so the assigned mode costs least unless a lower one ties."""
    rng = np.random.default_rng(seed)
    bw = R.subsample(w, bits)
    noise = rng.integers(0, 256, (h * w, 3))
    fresh = rng.integers(0, keep, h * w) == 0
    px = [0] * (h * w)
    for i in range(h * w):
        y, x = divmod(i, w)
        rnd = 0xff000000 | int(noise[i, 0]) << 16 | int(noise[i, 1]) << 8 | int(noise[i, 2])
        m = block_modes[((y >> bits) * bw + (x >> bits)) % len(block_modes)]
        if y == 0 or x == 0 or (fresh[i] and m != 0):
            px[i] = rnd
        else:
            px[i] = R.predict(m, px[i - 1], px[i - w], px[i - w - 1], px[i - w + 1])
    return ungather(np.array(px, np.uint32), h, w)


def large_frame():
    return P.large_frame()


def targeted_frames():
    """name -> (BGR frame, predictor_bits), each with one property the encoder can get wrong; tests/test_webp_encode_host.py asserts the
    properties on the rule book's taps."""
    rng = np.random.default_rng(5)
    out = {}
    out["tiny_1x1"] = (np.array([[[3, 1, 2]]], np.uint8), 4)
    out["row_1x9"] = (rng.integers(0, 256, (1, 9, 3), dtype=np.uint8), 4)
    out["column_9x1"] = (rng.integers(0, 256, (9, 1, 3), dtype=np.uint8), 4)
    out["width_2"] = (P.make_frame("photo", 37, 2, 1), 4)
    out["block_16x16"] = (P.make_frame("photo", 16, 16, 2), 4)
    out["edge_17x33"] = (P.make_frame("photo", 17, 33, 3), 4)
    out["edge_33x18"] = (P.make_frame("ramp", 33, 18), 4)
    out["row_16384"] = (one_row(rng.integers(0, 4, 16384).astype(np.uint32) * 0x010101), 4)
    out["column_16384"] = (one_column(rng.integers(0, 3, 16384).astype(np.uint32) * 0x010001), 4)
    out["runs_a"] = (one_row(runs_of([2, 3, 4095, 4096])), 4)           # 4095 and 4096 start inside a chunk of 1024 and end in a later one
    out["runs_b"] = (one_column(runs_of([4097, 4098])), 4)              # distance code 2 on an image one pixel wide
    out["runs_c"] = (one_row(runs_of([2 * 4096 + 3])), 4)
    out["flat"] = (np.full((48, 56, 3), (13, 200, 77), np.uint8), 4)    # one run across every row end and chunk
    out["black_1x3"] = (np.zeros((1, 3, 3), np.uint8), 4)               # three literals 0: all five codes have one symbol
    out["black_7x9"] = (np.zeros((7, 9, 3), np.uint8), 4)               # the literal 0 and one length symbol: a normal code of two symbols
    out["two_literals"] = (one_row(np.array([0x030405, 0x090807], np.uint32)), 4)      # simple codes of two symbols
    for terms in (16, 17, 18):                                          # 17 and 18: the tree is deeper than 15 bits before the repair
        out["fibonacci_%d" % terms] = (green_counts(fibonacci_counts(terms)), 4)
    out["tr_edge"] = (synth(35, 64, 4, [1, 2, 3, 4, 6, 5, 7, 8, 9, 11, 12, 10], 21), 4)      # modes 3, 5, 9, 10 in the last, 3 pixel wide block column
    out["all_modes"] = (synth(64, 64, 4, list(range(14)) + [13, 0], 22), 4)      # and its code-length code needs more than 7 bits before the repair
    out["clamping"] = (synth(48, 32, 4, [11, 12, 13], 23, keep=3), 4)
    g = np.zeros((5, 7, 3), np.uint8)                                   # red and blue below green: subtract-green wraps
    g[..., 1], g[..., 0], g[..., 2] = 200, np.arange(7) * 3, 10
    out["below_green"] = (g, 4)
    out["bits_2"] = (P.make_frame("photo", 11, 13, 4), 2)
    out["bits_9"] = (P.make_frame("ramp", 3, 600), 9)
    out["noise"] = (rng.integers(0, 256, (40, 40, 3), dtype=np.uint8), 4)
    return out


def smooth_frame(h, w):
    """Smooth structure without noise: where the predictors beat PNG's Sub filter by a wide margin."""
    y, x = np.mgrid[0:h, 0:w]
    ch = [128 + 70 * np.sin(x / (23.0 + 7 * c) + c) * np.cos(y / (31.0 - 5 * c)) + 30 * np.sin((x + 2 * y) / 9.1 + c) for c in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


FIXTURE_SIZES = [(1, 1), (1, 37), (29, 1), (2, 2), (8, 8), (17, 19), (33, 47), (64, 64)]      # h x w
FIXTURE_KINDS = ("noise", "flat", "ramp", "photo", "blocks", "smooth")


def fixture_frames():
    """name -> (frame, predictor_bits): the small frames of tests/golden/webp_encode_cases.npz."""
    out = {}
    for si, (h, w) in enumerate(FIXTURE_SIZES):
        for ki, kind in enumerate(FIXTURE_KINDS):
            frame = smooth_frame(h, w) if kind == "smooth" else P.make_frame(kind, h, w, seed=100 * si + ki)
            out["%dx%d_%s_bits4" % (h, w, kind)] = (frame, 4)
            if (h, w) == (33, 47):
                out["%dx%d_%s_bits2" % (h, w, kind)] = (frame, 2)
                out["%dx%d_%s_bits3" % (h, w, kind)] = (frame, 3)
    return out
