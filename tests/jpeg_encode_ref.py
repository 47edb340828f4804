"""NumPy restatement of libjpeg's baseline encoder with its defaults as Pillow drives it (jpeg_set_quality(q, force_baseline), JDCT_ISLOW,
standard Huffman tables, optimize off, JFIF 1.01 header): BGR uint8 frame in, file bytes out.  All arithmetic is integer.  The rules and the
libjpeg file each comes from:

  1. colour (jccolor.c rgb_ycc_convert, 16-bit fixed point; frames are BGR, so channel 2 is R):
       Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
       Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
       Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
  2. padding and 4:2:0 downsampling (jcprepct.c pre_process_data, jcsample.c h2v2_downsample): horizontally the INPUT is widened to
     width_in_blocks * 8 * h columns by repeating the last column; vertically the input is padded only to an even number of rows; then
     (a + b + c + d + bias) >> 2 with the bias alternating 1, 2, 1, 2 ... along the output row; the DOWNSAMPLED rows are then repeated down
     to height_in_blocks * 8.  (Repeating input rows to a multiple of 16 instead is wrong for every even height that is no multiple of 16.)
     Y and 4:4:4 planes are padded by plain edge repetition.
  3. forward DCT: jfdctint.c jpeg_fdct_islow on samples - 128 (CONST_BITS 13, PASS1_BITS 2); its output is 8 times the DCT.
  4. quantisation (jcdctmgr.c forward_DCT): divisor q * 8, |c| rounded with (|c| + divisor / 2) / divisor, sign restored.  Tables
     (jcparam.c jpeg_set_quality): scale 5000 / q below 50, 200 - 2 q from 50; (base * scale + 50) / 100 clamped to 1..255.
  5. block order and dummy blocks (jccoefct.c compress_data): MCUs in raster order, in 4:2:0 the four Y blocks, then Cb, then Cr.  A
     component has ceil(w * h_samp / (8 * h_max)) real block columns (likewise rows); MCU positions beyond them hold dummy blocks: all AC
     zero, DC equal to the DC of the block coded just before it in the same MCU (so the DC difference is 0: the DC code of category 0 + EOB).
  6. entropy coding (jchuff.c encode_one_block, std_huff_tables of jcparam.c): DC difference per component across the whole scan; ZRL
     (0xF0) for runs above 15; EOB unless coefficient 63 is non-zero; negative values sent as v - 1 in `size` bits; after the last block
     the partial byte is filled with 1-bits; every 0xFF byte of the stream (a fill byte included) is followed by 0x00; no restart markers.
  7. file (jcmarker.c): SOI, APP0 JFIF 1.01 (units 0, density 1 x 1), DQT luma, DQT chroma, SOF0, DHT DC 0, AC 0, DC 1, AC 1, SOS, the
     scan, EOI.

encode(frame, quality, subsampling) returns the file; with taps=dict it also leaves the stages there, so that a mismatch names its stage:
  ycc       [h, w, 3] uint8 (Y, Cb, Cr)                    planes    the three padded (and downsampled) planes, uint8
  coef      per component int16 [block rows, block cols, 64] in zigzag order over the MCU-padded grid (dummy blocks as rule 5 defines them)
  real      per component bool [block rows, block cols]: False for a dummy block
  coded     int16 [n blocks, 64]: the blocks in the order they are coded      coded_comp   int [n blocks]: each one's component
  bits      int32 [n blocks]: bits each block costs         stream    the entropy-coded bytes before stuffing (last byte filled)
  scan      the stuffed bytes                               header    everything in front of the scan
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int64)

# jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl (natural order)
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  np.int64)
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32, np.int64)

# jcparam.c std_huff_tables: (bits[1..16], values)
_AC_TAIL = [16 * r + s for r in range(16) for s in range(1, 11)]      # not the order of the tables: only used to check them below
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
            130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
            90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
            149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
            198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244,
            245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
              10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87,
              88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138,
              146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
              194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234,
              242, 243, 244, 245, 246, 247, 248, 249, 250])
assert sorted(AC_LUMA[1]) == sorted(AC_CHROMA[1]) == sorted(_AC_TAIL + [0, 240])


def quant_table(base, quality):
    """jpeg_set_quality -> jpeg_add_quant_table with force_baseline (natural order)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * scale + 50) // 100, 1, 255)


def huff_codes(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl -> (code [256], length [256]); length 0: the symbol has no code."""
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], size[vals[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, size


def color(frame):
    """Rule 1: BGR [h, w, 3] -> YCbCr [h, w, 3]."""
    f = frame.astype(np.int64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1).astype(np.uint8)


def _edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def geometry(w, h, hs):
    """(mcux, mcuy, per component (real block cols, real block rows, block cols of the MCU grid, block rows of it))."""
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * hs))
    comps = []
    for s in (hs, 1, 1):
        comps.append((-(-(w * s) // (8 * hs)), -(-(h * s) // (8 * hs)), mcux * s, mcuy * s))
    # ceil(w * s / hs) samples, then ceil(/ 8) blocks: the nested ceilings equal the single one
    return mcux, mcuy, comps


def planes(ycc, hs):
    """Rule 2: the three component planes, each padded to whole real blocks."""
    h, w, _ = ycc.shape
    _, _, comps = geometry(w, h, hs)
    out = [_edge(ycc[..., 0], 8 * comps[0][1], 8 * comps[0][0])]
    for c in (1, 2):
        bc, br = comps[c][0], comps[c][1]
        if hs == 1:
            out.append(_edge(ycc[..., c], 8 * br, 8 * bc))
            continue
        p = _edge(ycc[..., c], h + (h & 1), 16 * bc).astype(np.int64)     # columns to width_in_blocks * 8 * h, rows to an even count
        bias = np.tile(np.array([1, 2], np.int64), 4 * bc)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_edge(d.astype(np.uint8), 8 * br, 8 * bc))             # the downsampled rows repeated
    return out


_F = dict(F_0_298631336=2446, F_0_390180644=3196, F_0_541196100=4433, F_0_765366865=6270, F_0_899976223=7373, F_1_175875602=9633,
          F_1_501321110=12299, F_1_847759065=15137, F_1_961570560=16069, F_2_053119869=16819, F_2_562915447=20995, F_3_072711026=25172)


def _fdct_1d(d, first):
    """One pass of jpeg_fdct_islow over the last axis of d [..., 8]."""
    C, P = 13, 2

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << P, (t10 - t11) << P
        n = C - P
    else:
        o[0], o[4] = descale(t10 + t11, P), descale(t10 - t11, P)
        n = C + P
    z1 = (t12 + t13) * _F["F_0_541196100"]
    o[2] = descale(z1 + t13 * _F["F_0_765366865"], n)
    o[6] = descale(z1 - t12 * _F["F_1_847759065"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F["F_1_175875602"]
    t4, t5, t6, t7 = t4 * _F["F_0_298631336"], t5 * _F["F_2_053119869"], t6 * _F["F_3_072711026"], t7 * _F["F_1_501321110"]
    z1, z2 = -z1 * _F["F_0_899976223"], -z2 * _F["F_2_562915447"]
    z3, z4 = -z3 * _F["F_1_961570560"] + z5, -z4 * _F["F_0_390180644"] + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(plane, qtab):
    """Rules 3 and 4: a plane of whole blocks -> int16 [block rows, block cols, 64] quantised coefficients in zigzag order."""
    br, bc = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.astype(np.int64).reshape(br, 8, bc, 8).transpose(0, 2, 1, 3) - 128      # [br, bc, row, col]
    blk = _fdct_1d(blk, True)                                      # rows
    blk = _fdct_1d(blk.swapaxes(-1, -2), False).swapaxes(-1, -2)   # columns
    c = blk.reshape(br, bc, 64)
    div = qtab.astype(np.int64) * 8
    qz = (np.abs(c) + (div >> 1)) // div
    return (np.sign(c) * qz)[..., ZIGZAG].astype(np.int16)


def coded_blocks(coefs, w, h, hs):
    """Rule 5: the blocks of the three components (each over its real blocks) in coded order.
    -> (coded int16 [N, 64], component [N], real bool [N], per component (coef over the MCU grid, real mask))."""
    mcux, mcuy, comps = geometry(w, h, hs)
    grids, masks, index = [], [], []
    for c in range(3):
        bc, br, gc, gr = comps[c]
        g = np.zeros((gr, gc, 64), np.int16)
        g[:br, :bc] = coefs[c]
        m = np.zeros((gr, gc), bool)
        m[:br, :bc] = True
        grids.append(g)
        masks.append(m)
    my, mx = np.meshgrid(np.arange(mcuy), np.arange(mcux), indexing="ij")
    comp, by, bx = [], [], []
    for c, s in enumerate((hs, 1, 1)):
        for v in range(s):
            for hh in range(s):
                comp.append(np.full(mx.shape, c))
                by.append(my * s + v)
                bx.append(mx * s + hh)
    comp, by, bx = (np.stack(a, -1).reshape(-1) for a in (comp, by, bx))       # [mcuy, mcux, blocks per MCU] flattened: the coded order
    real = np.array([masks[c][y, x] for c, y, x in zip(comp, by, bx)])
    coded = np.stack([grids[c][y, x] for c, y, x in zip(comp, by, bx)]).astype(np.int16)
    for i in np.flatnonzero(~real):                                # a dummy block: the DC of the block coded just before it (same MCU, same component)
        coded[i, 0] = coded[i - 1, 0]
        grids[comp[i]][by[i], bx[i], 0] = coded[i, 0]
    return coded, comp, real, grids, masks


def _bitlen(a):
    n = np.zeros(a.shape, np.int64)
    a = a.copy()
    while a.any():
        n += a > 0
        a >>= 1
    return n


def entropy(coded, comp):
    """Rule 6 without the stuffing: (bits per block int32 [N], the bytes of the stream with the last one filled with 1-bits).
    Vectorised: every coefficient owns 4 token slots (up to three ZRL, then run/size + value bits), every block one more for EOB."""
    N = coded.shape[0]
    v = coded.astype(np.int64)
    chroma = comp > 0
    dc = v[:, 0].copy()
    for c in range(3):                                             # DC difference per component across the scan
        i = np.flatnonzero(comp == c)
        dc[i] = np.diff(v[i, 0], prepend=0)
    v[:, 0] = dc
    mag = np.abs(v)
    size = _bitlen(mag)
    val = np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    pos = np.arange(64)
    nz = v != 0
    nz[:, 0] = True                                                # the DC slot always ends a run
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)     # position of the latest coded coefficient up to here
    prev = np.concatenate([np.zeros((N, 1), np.int64), last[:, :-1]], 1)
    run = np.where(nz, pos - prev - 1, 0)
    run[:, 0] = 0
    tabs = [huff_codes(*t) for t in (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA)]
    code = np.zeros((N, 65, 4), np.int64)
    length = np.zeros((N, 65, 4), np.int64)
    for ch in (0, 1):
        rows = np.flatnonzero(chroma == bool(ch))
        dcode, dlen = tabs[ch]
        acode, alen = tabs[2 + ch]
        s0 = size[rows, 0]
        code[rows, 0, 3] = (dcode[s0] << s0) | val[rows, 0]
        length[rows, 0, 3] = dlen[s0] + s0
        r, s, a = run[rows, 1:], size[rows, 1:], nz[rows, 1:]
        sym = ((r & 15) << 4) | s
        code[rows, 1:64, 3] = np.where(a, (acode[sym] << s) | val[rows, 1:], 0)
        length[rows, 1:64, 3] = np.where(a, alen[sym] + s, 0)
        for k in range(3):                                         # ZRL codes in front
            z = a & ((r >> 4) > k)
            code[rows, 1:64, k] = np.where(z, acode[0xF0], 0)
            length[rows, 1:64, k] = np.where(z, alen[0xF0], 0)
        eob = v[rows, 63] == 0
        code[rows, 64, 3] = np.where(eob, acode[0], 0)
        length[rows, 64, 3] = np.where(eob, alen[0], 0)
    assert length[:, :64, 3][nz].min() > 0                          # every coded symbol has a code
    bits = length.reshape(N, -1).sum(1)
    fl, fc = length.reshape(-1), code.reshape(-1)
    keep = fl > 0
    fl, fc = fl[keep], fc[keep]
    total = int(fl.sum())
    start = np.cumsum(fl) - fl
    j = np.arange(total) - np.repeat(start, fl)                    # bit index inside its token, most significant first
    stream = ((np.repeat(fc, fl) >> (np.repeat(fl, fl) - 1 - j)) & 1).astype(np.uint8)
    stream = np.concatenate([stream, np.ones(-total % 8, np.uint8)])
    return bits.astype(np.int32), np.packbits(stream)


def stuff(stream):
    """0x00 after every 0xFF."""
    return np.insert(stream, np.flatnonzero(stream == 0xFF) + 1, 0)


def header(w, h, hs, qluma, qchroma):
    """Rule 7: everything in front of the scan."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, bytes([0]) + bytes(qluma[ZIGZAG].astype(np.uint8))) + seg(0xDB, bytes([1]) + bytes(qchroma[ZIGZAG].astype(np.uint8)))
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 16 * hs + hs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(frame, quality=95, subsampling="4:2:0", taps=None):
    """BGR uint8 [h, w, 3] -> the bytes of the JPEG file libjpeg writes for it."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and frame.shape[0] > 0 and frame.shape[1] > 0
    hs = {"4:2:0": 2, "4:4:4": 1}[subsampling]
    h, w, _ = frame.shape
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    ycc = color(frame)
    pl = planes(ycc, hs)
    coefs = [fdct_quant(p, q) for p, q in zip(pl, (ql, qc, qc))]
    coded, comp, real, grids, masks = coded_blocks(coefs, w, h, hs)
    bits, stream = entropy(coded, comp)
    scan = stuff(stream)
    head = header(w, h, hs, ql, qc)
    if taps is not None:
        taps.update(ycc=ycc, planes=pl, coef=grids, real=masks, coded=coded, coded_comp=comp, coded_real=real, bits=bits, stream=stream,
                    scan=scan, header=head, quant=(ql, qc))
    return head + scan.tobytes() + b"\xff\xd9"


# ---------------------------------------------------------------- test content (integer arithmetic only: the same pixels on every machine)

def make_frame(kind, h, w, seed=0):
    """BGR uint8 [h, w, 3]: "random" noise, a smooth "ramp" (long zero runs at low quality) or "saturated" 0 / 255 noise (the largest
    coefficients, DC category 11 and AC size 10 at quality 100, and 0xFF bytes in the stream)."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 5 + y * 2) % 256, (y * 7) % 256, (x * 3 + y) % 256], -1).astype(np.uint8)


def smooth_frame(h, w):
    """A large smooth picture: slow gradients with a coarse integer texture."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x // 3 + y // 5) % 256, (y // 2 + ((x * x + y * y) >> 11)) % 256, (x // 4 + y // 7 + ((x * y) >> 10)) % 256], -1).astype(np.uint8)
