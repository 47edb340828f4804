"""The rule book of the lossy WebP (VP8) ENCODER in NumPy and plain Python: what maf-yolo_amd/webp_lossy_encode.py and csrc/vp8_encode.hip must
write, byte for byte.  It stands on webp_lossy_ref.py (the bool encoder, the syntax walkers, predict_block, dequantise, idct, iwht) and
webp_lossy_tables.py and changes neither.  tools/make_golden_webp_lossy_encode.py asserts, for every fixture, that Pillow (libwebp) decodes
the file to what webp_lossy_ref.decode_stages returns and that a decoder's unfiltered planes are the reconstruction this encoder predicted from.

  encode(bgr, base_q, filter_level=None, log2_parts=3, taps=None) -> the file's bytes
  taps: planes (the padded Y, U, V that went in), ymodes, uvmodes, levels int16 [mb][25][16] (zigzag order, block 24 = Y2), skips, recon (the
        unfiltered reconstruction, padded), part_sizes (the first partition, then the token partitions), frame (webp_lossy_ref.Frame).

The profile: RIFF / WEBP, one `VP8 ` chunk, one key frame; no segments, no filter deltas, sharpness 0, the normal filter, every dq 0; every
macroblock predicted 16x16, the luma mode (and the chroma mode, over U and V together) the one of DC, TM, V, H with the lowest sum of squared
differences against the prediction from the RECONSTRUCTED neighbours (ties: the lowest number); libwebp's integer forward DCT and WHT;
level = sign(c) * min((|c| + (q >> 1)) // q, 2047); default probabilities; skips where use_skip pays.
The colour conversion is this project's rule (integer BT.601 on the plain 2x2 sum), not libwebp's gamma-aware one.
"""
import numpy as np

import webp_lossy_ref as R
from webp_lossy_tables import AC_Q, BANDS, CAT3456, COEFF_PROBA0, ZIGZAG

HEADER_BOOLS = 1094          # of the first partition in front of the macroblock modes: 29 header bools, 1056 update flags, use_skip and skip_proba
MODE_BOOLS = 8               # per macroblock at the most (skip 1, i16 flag 1, luma mode 2, chroma mode 3: seven)
FLUSH_BYTES = 4              # BoolEncoder.finish appends four bytes


def quality_to_base_q(quality):
    """libwebp's curve from `quality` to its quantiser index (before its segment and SNS adjustments)."""
    c = quality / 100.0
    c = 2.0 * c / 3.0 if c < 0.75 else 2.0 * c - 1.0
    return int(127.0 * (1.0 - c ** (1.0 / 3.0)))


def default_filter_level(base_q):
    return min(63, int(AC_Q[base_q]) >> 2)


def bgr_to_yuv(bgr):
    """uint8 [h, w, 3] BGR -> Y [16 mbh, 16 mbw], U, V [8 mbh, 8 mbw] uint8: the last column and row replicated out to whole macroblocks."""
    h, w = bgr.shape[:2]
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    p = np.pad(bgr.astype(np.int64), ((0, 16 * mbh - h), (0, 16 * mbw - w), (0, 0)), mode="edge")
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = (16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16

    def s4(c):
        return c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    r4, g4, b4 = s4(r), s4(g), s4(b)
    u = (-9719 * r4 - 19081 * g4 + 28800 * b4 + (128 << 18) + (1 << 17)) >> 18
    v = (28800 * r4 - 24116 * g4 - 4684 * b4 + (128 << 18) + (1 << 17)) >> 18
    assert 0 <= min(y.min(), u.min(), v.min()) and max(y.max(), u.max(), v.max()) <= 255
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def fdct(res):
    """The 4 x 4 residual [row][column] -> 16 coefficients in raster order (libwebp's FTransform)."""
    d = [[int(v) for v in row] for row in res]
    tmp = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = d[i][0] + d[i][3], d[i][1] + d[i][2], d[i][1] - d[i][2], d[i][0] - d[i][3]
        tmp[4 * i:4 * i + 4] = (a0 + a1) * 8, (a2 * 2217 + a3 * 5352 + 1812) >> 9, (a0 - a1) * 8, (a3 * 2217 - a2 * 5352 + 937) >> 9
    out = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = tmp[i] + tmp[12 + i], tmp[4 + i] + tmp[8 + i], tmp[4 + i] - tmp[8 + i], tmp[i] - tmp[12 + i]
        out[i] = (a0 + a1 + 7) >> 4
        out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0)
        out[8 + i] = (a0 - a1 + 7) >> 4
        out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16
    return out


def fwht(dc):
    """The DC of the 16 luma blocks (raster order) -> the 16 Y2 coefficients in raster order (libwebp's FTransformWHT)."""
    tmp = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = dc[4 * i] + dc[4 * i + 2], dc[4 * i + 1] + dc[4 * i + 3], dc[4 * i + 1] - dc[4 * i + 3], dc[4 * i] - dc[4 * i + 2]
        tmp[4 * i:4 * i + 4] = a0 + a1, a3 + a2, a3 - a2, a0 - a1
    out = [0] * 16
    for i in range(4):
        a0, a1, a2, a3 = tmp[i] + tmp[8 + i], tmp[4 + i] + tmp[12 + i], tmp[4 + i] - tmp[12 + i], tmp[i] - tmp[8 + i]
        out[i], out[4 + i], out[8 + i], out[12 + i] = (a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1
    return out


def quantise(c, q):
    a = min((abs(c) + (q >> 1)) // q, 2047)
    return -a if c < 0 else a


def _nz(lv):
    return max([i + 1 for i in range(16) if lv[i]], default=0)


def _best_mode(P, S, mx, my, n, planes=1):
    """The mode of DC, TM, V, H with the lowest squared error between the source blocks S and the predictions inside the planes P."""
    best, best_sse, preds = 0, None, None
    for mode in (R.DC_PRED, R.TM_PRED, R.V_PRED, R.H_PRED):
        sse, ws = 0, []
        for Pk, Sk in zip(P, S):
            W = R._work(Pk, mx, my, n, 0)
            R.predict_block(mode, W, n, mx, my)
            pred = W[1:n + 1, 1:n + 1]
            sse += int(((Sk - pred) ** 2).sum())
            ws.append(pred.copy())
        if best_sse is None or sse < best_sse:
            best, best_sse, preds = mode, sse, ws
    return best, preds


def analyse(planes, f):
    """Modes, levels and the reconstruction of every macroblock of Frame f (its header is set) -> the unfiltered planes (int32, padded)."""
    Ys, Us, Vs = (p.astype(np.int32) for p in planes)
    mbw, mbh = f.mbw, f.mbh
    Y, U, V = np.zeros_like(Ys), np.zeros_like(Us), np.zeros_like(Vs)
    q = R.quantisers(f)[0]
    y1dc, y1ac, y2dc, y2ac, uvdc, uvac, _ = q
    f.mbs = []
    for my in range(mbh):
        for mx in range(mbw):
            mb = dict(i4=0, segment=0, skip=0)
            src = Ys[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
            mb["ymode"], (pred,) = _best_mode((Y,), (src,), mx, my, 16)
            lv = [[0] * 16 for _ in range(25)]
            dcs = [0] * 16
            for b in range(16):
                r0, c0 = 4 * (b >> 2), 4 * (b & 3)
                co = fdct(src[r0:r0 + 4, c0:c0 + 4] - pred[r0:r0 + 4, c0:c0 + 4])
                dcs[b] = co[0]
                for n in range(1, 16):
                    lv[b][n] = quantise(co[ZIGZAG[n]], y1ac)
            y2 = fwht(dcs)
            for n in range(16):
                lv[24][n] = quantise(y2[ZIGZAG[n]], y2ac if n else y2dc)
            csrc = (Us[8 * my:8 * my + 8, 8 * mx:8 * mx + 8], Vs[8 * my:8 * my + 8, 8 * mx:8 * mx + 8])
            mb["uvmode"], cpred = _best_mode((U, V), csrc, mx, my, 8)
            for ch in (0, 1):
                for b in range(4):
                    r0, c0 = 4 * (b >> 1), 4 * (b & 1)
                    co = fdct(csrc[ch][r0:r0 + 4, c0:c0 + 4] - cpred[ch][r0:r0 + 4, c0:c0 + 4])
                    for n in range(16):
                        lv[16 + 4 * ch + b][n] = quantise(co[ZIGZAG[n]], uvac if n else uvdc)
            mb["levels"], mb["nz"] = lv, [_nz(b) for b in lv]
            co = R.dequantise(f, mb, q)                       # what a decoder will see
            for b in range(16):
                r0, c0 = 4 * (b >> 2), 4 * (b & 3)
                Y[16 * my + r0:16 * my + r0 + 4, 16 * mx + c0:16 * mx + c0 + 4] = np.clip(pred[r0:r0 + 4, c0:c0 + 4] + R.idct(co[b]), 0, 255)
            for ch, P in ((0, U), (1, V)):
                for b in range(4):
                    r0, c0 = 4 * (b >> 1), 4 * (b & 1)
                    P[8 * my + r0:8 * my + r0 + 4, 8 * mx + c0:8 * mx + c0 + 4] = np.clip(cpred[ch][r0:r0 + 4, c0:c0 + 4] + R.idct(co[16 + 4 * ch + b]), 0, 255)
            mb["zero"] = not any(mb["nz"])
            f.mbs.append(mb)
    return Y, U, V


def write(f):
    """Frame -> (the payload of the `VP8 ` chunk, the sizes of the first partition and of the token partitions): webp_lossy_ref.write_frame."""
    io0 = R.BoolEncoder()
    R.walk_header(io0, f)
    R.walk_header_tail(io0, f)
    ios = [R.BoolEncoder() for _ in range(1 << f.log2_parts)]
    R.walk_frame(io0, ios, f, False)
    first = io0.finish()
    parts = [io.finish() for io in ios]
    tag = 1 << 4 | len(first) << 5
    out = bytes([tag & 255, tag >> 8 & 255, tag >> 16 & 255]) + b"\x9d\x01\x2a" + bytes([f.width & 255, f.width >> 8, f.height & 255, f.height >> 8])
    out += first + b"".join(len(p).to_bytes(3, "little") for p in parts[:-1]) + b"".join(parts)
    return out, [len(first)] + [len(p) for p in parts]


def encode(bgr, base_q, filter_level=None, log2_parts=3, taps=None):
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3 and 0 <= base_q <= 127 and 0 <= log2_parts <= 3
    f = R.Frame()
    f.height, f.width = bgr.shape[:2]
    assert 1 <= f.width <= 16383 and 1 <= f.height <= 16383
    f.base_q = int(base_q)
    f.level = default_filter_level(f.base_q) if filter_level is None else int(filter_level)
    assert 0 <= f.level <= 63
    f.log2_parts = min(int(log2_parts), f.mbh.bit_length() - 1)          # every partition owns a macroblock row: libwebp refuses an empty last one
    planes = bgr_to_yuv(bgr)
    recon = analyse(planes, f)
    total, skips = len(f.mbs), sum(mb["zero"] for mb in f.mbs)
    f.skip_proba = (total - skips) * 255 // total
    f.use_skip = int(f.skip_proba < 250)
    if not f.use_skip:
        f.skip_proba = 0
    for mb in f.mbs:
        mb["skip"] = int(f.use_skip and mb["zero"])
    payload, sizes = write(f)
    assert sizes[0] < 1 << 19
    if taps is not None:
        taps.update(planes=planes, recon=tuple(p.astype(np.uint8) for p in recon), ymodes=np.array([mb["ymode"] for mb in f.mbs], np.uint8),
                    uvmodes=np.array([mb["uvmode"] for mb in f.mbs], np.uint8), skips=np.array([mb["skip"] for mb in f.mbs], np.uint8),
                    levels=np.array([mb["levels"] for mb in f.mbs], np.int16), part_sizes=sizes, frame=f)
    return R.riff(payload)


# ---------------------------------------------------------------- the derived worst case

def bool_shifts(prob, bit):
    """The most renormalisation shifts (= bits written) one bool of probability `prob` and value `bit` can cost, over every range 128 .. 255."""
    worst = 0
    for r in range(128, 256):
        split = 1 + (((r - 1) * prob) >> 8)
        new = r - split if bit else split
        worst = max(worst, 7 - (new.bit_length() - 1))
    return worst


def _large_worst(p):
    """The dearest path through the tokens above 1 (the bits behind p[2] = 1, without the sign)."""
    c = bool_shifts
    small = c(p[3], 0) + max(c(p[4], 0), c(p[4], 1) + max(c(p[5], 0), c(p[5], 1)))
    cat1 = c(p[7], 0) + max(c(159, 0), c(159, 1))
    cat2 = c(p[7], 1) + max(c(165, 0), c(165, 1)) + max(c(145, 0), c(145, 1))
    mid = c(p[3], 1) + c(p[6], 0) + max(cat1, cat2)
    big = 0
    for cat in range(4):
        bit1 = cat >> 1
        extra = sum(max(c(pr, 0), c(pr, 1)) for pr in CAT3456[cat])
        big = max(big, c(p[8], bit1) + c(p[9 + bit1], cat & 1) + extra)
    return max(small, mid, c(p[3], 1) + c(p[6], 1) + big)


def block_worst_bits(t, first):
    """The most bits the tokens of one block of type t that starts at coefficient `first` can take, whatever its levels and context."""
    c = bool_shifts
    P = COEFF_PROBA0[t]
    # cost[n][ctx][after a zero token]: from coefficient n on
    cost = [[[0, 0] for _ in range(3)] for _ in range(17)]
    for n in range(15, first - 1, -1):
        for ctx in range(3):
            p = [int(v) for v in P[BANDS[n]][ctx]]
            nxt = cost[n + 1]
            token = max(c(p[1], 0) + nxt[0][1],                                    # a zero (the next bool skips p[0])
                        c(p[1], 1) + c(p[2], 0) + 1 + nxt[1][0],                   # one, its sign
                        c(p[1], 1) + c(p[2], 1) + _large_worst(p) + 1 + nxt[2][0])
            cost[n][ctx][1] = token
            cost[n][ctx][0] = max(c(p[0], 0), c(p[0], 1) + token)
    return max(cost[first][ctx][0] for ctx in range(3))


def mb_worst_bits():
    """One macroblock's tokens: the Y2 block, 16 luma blocks from coefficient 1, 8 chroma blocks."""
    return block_worst_bits(1, 0) + 16 * block_worst_bits(0, 1) + 8 * block_worst_bits(2, 0)
