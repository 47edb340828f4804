"""NumPy restatement of libjpeg's baseline decoder with its defaults (JDCT_ISLOW, fancy upsampling), the rule csrc/jpeg_decode.hip
follows bit for bit.  Pillow (libjpeg-turbo) is the judge of this file (tests/test_jpeg_host.py); this file is the judge of the kernels
and provides their intermediate taps (coefficients, planes).  The marker walk is maf_yolo_amd.jpeg.parse (tested on its own); everything
after it is restated here, independently of the device tables.

  entropy      jdhuff.c decode_mcu: canonical Huffman codes read bit by bit (mincode / maxcode per length), HUFF_EXTEND, DC prediction per
               component reset at every restart interval, AC runs with ZRL (0xF0) and EOB (0x00), coefficients de-zigzagged (jutils.c
               jpeg_natural_order); 0xFF00 unstuffed; the interleaved MCU order of jdcoefct.c (per component v x h blocks, row-major)
  idct         jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, columns then rows, DESCALE with rounding, the output through
               the range-limit table of jdmaster.c prepare_range_limit_table indexed with & 1023 (it wraps, it does not clamp, past +-512)
  planes       every block of every MCU is decoded, so a component plane is padded to whole MCUs (jdcoefct.c); the image's own rows and
               columns are what jdmainct.c hands on: the upsampler never reads past column downsampled_width - 1 (ceil(w / 2)) and
               the context rows above the first / below the last real row (downsampled_height - 1) repeat that row
  upsample     jdsample.c: h2v1_fancy_upsample (3/4, 1/4 with the +1 / +2 alternating rounding, edge columns copied) and
               h2v2_fancy_upsample (column sums 3 * near row + far row, then (3 * this + neighbour + 8 | 7) >> 4); both ONLY when
               downsampled_width > 2, otherwise the box replication of h2v1_upsample / h2v2_upsample
  colour       jdcolor.c build_ycc_rgb_table / ycc_rgb_convert: SCALEBITS 16, FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414),
               clamped to [0, 255]; written B, G, R.  A one-component file repeats its gray value (cv2.imread's default flag)
"""
import numpy as np

from maf_yolo_amd import jpeg as J

FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865 = 2446, 3196, 4433, 6270
FIX_0_899976223, FIX_1_175875602, FIX_1_501321110, FIX_1_847759065 = 7373, 9633, 12299, 15137
FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026 = 16069, 16819, 20995, 25172
CONST_BITS, PASS1_BITS = 13, 2


class _Bits:
    """MSB-first bit reader over one restart interval's bytes with 0xFF00 unstuffed; past the end it feeds zeros and counts them."""

    def __init__(self, data):
        a = np.frombuffer(data, np.uint8)
        keep = np.ones(len(a), bool)
        ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, np.int64)
        keep[ff[a[ff + 1] == 0] + 1] = False
        self.bytes = a[keep].tolist()
        self.pos = 0          # in bits
        self.n = 8 * len(self.bytes)

    def bit(self):
        p = self.pos
        self.pos += 1
        if p >= self.n:
            return 0
        return (self.bytes[p >> 3] >> (7 - (p & 7))) & 1

    def get(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    @property
    def overrun(self):
        return self.pos > self.n


def _canon(bits, vals):
    """mincode, maxcode, valptr per code length (1..16) of a canonical Huffman table."""
    mincode, maxcode, valptr = [0] * 17, [-1] * 17, [0] * 17
    code = k = 0
    for l in range(1, 17):
        n = int(bits[l - 1])
        if n:
            valptr[l], mincode[l] = k, code
            code += n
            k += n
            maxcode[l] = code - 1
        code <<= 1
    return mincode, maxcode, valptr, [int(v) for v in vals]


def _sym(br, tab):
    mincode, maxcode, valptr, vals = tab
    code = 0
    for l in range(1, 17):
        code = (code << 1) | br.bit()
        if maxcode[l] >= 0 and code <= maxcode[l] and code >= mincode[l]:
            return vals[valptr[l] + code - mincode[l]]
    return None


def _extend(r, s):
    return r - (1 << s) + 1 if r < (1 << (s - 1)) else r


def coefficients(data, info=None):
    """Entropy decode -> (list of int16 [bh_c, bw_c, 64] natural-order coefficient arrays per component, status word)."""
    d = J._bytes(data)
    info = info or J.parse(d)
    nc, hs, vs, mcux, mcuy, _ = J.geometry(info)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int16) for h, v in samp]
    dct = [_canon(*info.huffman[(0, c.td)]) for c in info.components]
    act = [_canon(*info.huffman[(1, c.ta)]) for c in info.components]
    total = mcux * mcuy
    ri = info.restart_interval or total
    nl = -(-total // ri)
    total_status = 0
    zz = J.ZIGZAG.tolist()
    for k, (b0, b1) in enumerate(J._restart_ranges(d, info.scan, nl)):
        br = _Bits(d[b0:b1])
        pred = [0] * nc
        ok = True
        status = 0
        for m in range(k * ri, min((k + 1) * ri, total)):
            my, mx = divmod(m, mcux)
            for c, (h, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(h):
                        blk = coefs[c][my * v + by, mx * h + bx]
                        s = _sym(br, dct[c])
                        if s is None:
                            status |= J.STATUS_BAD_CODE
                            ok = False
                            break
                        diff = _extend(br.get(s), s) if s else 0
                        pred[c] += diff
                        blk[0] = ((pred[c] + 32768) & 0xFFFF) - 32768          # JCOEF is a short
                        kk = 1
                        while kk < 64:
                            rs = _sym(br, act[c])
                            if rs is None:
                                status |= J.STATUS_BAD_CODE
                                ok = False
                                break
                            r, s = rs >> 4, rs & 15
                            if s:
                                kk += r
                                if kk > 63:
                                    status |= J.STATUS_BAD_INDEX
                                    ok = False
                                    break
                                blk[zz[kk]] = _extend(br.get(s), s)
                                kk += 1
                            elif r == 15:
                                kk += 16
                            else:
                                break
                        if not ok:
                            break
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
        if br.overrun:                                      # zeros past the interval's end were consumed: that is the fault, whatever they decoded to
            status = J.STATUS_SHORT_SCAN
        total_status |= status
    return coefs, total_status


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, shift):
    """One 1-D pass of jpeg_idct_islow over the LAST axis of d (int64 [..., 8]) -> the 8 outputs, descaled by `shift`."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * FIX_0_541196100
    tmp2 = z1 + z3 * (-FIX_1_847759065)
    tmp3 = z1 + z2 * FIX_0_765366865
    z2, z3 = d[..., 0], d[..., 4]
    tmp0 = (z2 + z3) << CONST_BITS
    tmp1 = (z2 - z3) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * FIX_1_175875602
    tmp0 = tmp0 * FIX_0_298631336
    tmp1 = tmp1 * FIX_2_053119869
    tmp2 = tmp2 * FIX_3_072711026
    tmp3 = tmp3 * FIX_1_501321110
    z1 = z1 * (-FIX_0_899976223)
    z2 = z2 * (-FIX_2_562915447)
    z3 = z3 * (-FIX_1_961570560) + z5
    z4 = z4 * (-FIX_0_390180644) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([_descale(o, shift) for o in out], -1)


def range_limit(x):
    """sample_range_limit + CENTERJSAMPLE indexed with x & RANGE_MASK (jdmaster.c prepare_range_limit_table)."""
    v = x & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def idct_plane(coef, q):
    """int16 [bh, bw, 64] coefficients x uint16 [64] quantisation table -> the uint8 [8 bh, 8 bw] component plane."""
    bh, bw, _ = coef.shape
    d = (coef.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)          # [row u][column v]
    ws = _pass(d.transpose(0, 1, 3, 2), CONST_BITS - PASS1_BITS)                      # pass 1 runs down each column: -> [column][row]
    px = _pass(ws.transpose(0, 1, 3, 2), CONST_BITS + PASS1_BITS + 3)                 # pass 2 along each row
    return range_limit(px).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def planes(data, info=None):
    d = J._bytes(data)
    info = info or J.parse(d)
    coefs, status = coefficients(d, info)
    return [idct_plane(c, info.qtables[comp.tq]) for c, comp in zip(coefs, info.components)], status


def h2v1_fancy(p):
    """h2v1_fancy_upsample on int [rows, dw] -> [rows, 2 dw]."""
    prev = np.concatenate([p[:, :1], p[:, :-1]], 1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    return out


def h2v2_fancy(p):
    """h2v2_fancy_upsample on int [dh, dw] -> [2 dh, 2 dw]; the rows above the first and below the last repeat them (jdmainct.c)."""
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for v, far in ((0, up), (1, dn)):
        cs = 3 * p + far
        prev = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + prev + 8) >> 4
        out[v::2, 1::2] = (3 * cs + nxt + 7) >> 4
    return out


def upsample(plane, w, h, hs, vs):
    """A chroma plane (padded to whole MCUs) -> int [h, w] at full resolution by jdsample.c's default rules."""
    dw, dh = -(-w // hs), -(-h // vs)
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 2:
        if dw > 2:
            p = h2v2_fancy(p) if vs == 2 else h2v1_fancy(p)
        else:
            p = p.repeat(2, 1).repeat(vs, 0)
    return p[:h, :w]


def ycc_to_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data):
    """File bytes -> uint8 [h, w, 3] BGR, what cv2.imread returns (EXIF rotation aside)."""
    d = J._bytes(data)
    info = J.parse(d)
    pl, status = planes(d, info)
    if status:
        raise J.MafError("jpeg_ref: " + J.status_text(status))
    w, h = info.width, info.height
    y = pl[0][:h, :w]
    if len(pl) == 1:
        return np.repeat(y[:, :, None], 3, 2)
    _, hs, vs, _, _, _ = J.geometry(info)
    return ycc_to_bgr(y, upsample(pl[1], w, h, hs, vs), upsample(pl[2], w, h, hs, vs))
