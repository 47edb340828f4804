"""-m gpu: the forward (inference) kernels at their dispatch edges, straight through the C ABI (maf_op_launch), EXACTLY where the arithmetic allows it (cases and
references: tests/fwd_ref.py, checked by test_fwd_ref_host.py on the very tensors used here).

OP_CONV1X1 and OP_CONV3X3S2 on every (tile_p, tile_c, tile_k) conv_variants.conv_tiles lists for the case's shape — at its own pixel count and at 65536 pixels, where
the list holds the tile_p 2 / 4 entries too — plus the tiles a case names itself (the DMA ring on {1, 2} x {4, 6, 8}, CONV3_LDS / CONV3_WREG workgroup counts); OP_DWCONV on
the generic kernel (cost-model and explicit tiles), MAF_DW_DOT2, MAF_DW_PAIRS (waves 1 .. 8, staged stores) and MAF_DW_MFMA; OP_STEM; OP_SPPF_POOL; OP_BOTTLENECK (with and without the block's closing conv, and 66 launches
alternating two streams) and OP_CONV1DW; OP_STEM2; OP_HEADTAIL.

Every source is a channel slice of a wider buffer whose other channels, and the pixel before and after the map, are NaN; the slice sits at the front or the back of
its buffer in turn; a pixel-pair source is embedded in the pair layout (pack.pairs_from_nhwc); the sources of a multi-source conv and a twin's source are poisoned
buffers of their own.  Every output (the twin's, the pooled 1x1 branch's too) is a slice that holds NaN in a buffer that holds a sentinel elsewhere, which must come
back bit-identical.  No MAF_* override is set: the branches are reached by shape and tile fields, and fwd_ref.CASES names, beside each case, the branch it is there for.
Finite poison in place of NaN, and why: a source read through MAX — SRC_POOL2 and OP_SPPF_POOL — is poisoned with 2^15 (SPPF: the sentinel 12344, above every
input), because the hardware maximum returns the operand that is not NaN: a NaN neighbour would never show.  No kernel had to have its poison made finite for
reading channels past its slice: chunks past a source's last channel read chunk 0 of the slice itself (times zero weights).

Family E: torch.equal(got, ref.to(dtype)).  Family B (and the pooled branch, whose SiLU is hard-wired): op_ref's per-element bound, constants as they stand.  A
candidate the library refuses passes only if the launch returns non-zero and every output buffer still holds its poison and sentinel; the tally of accepted and
refused candidates per (op, variant) is asserted at the end of the file.

What ran on the MI355X (accepted launches per variant; every one of them passed; `twin`, `pooled`, `pairs-out`, `f32-out`, `fp32` are counted apart):
    OP_CONV1X1     generic 426 (+ 66 fp32, 32 twin, 26 f32-out), lds 146 (+ 14 twin), dma 102 (+ 12 twin), k4 (split-K) 56 (+ 8 twin, 6 f32-out, 4 fp32), stream 104,
                   streamlds 136 at tile_p 1 and 23 at tile_p 2 (+ 12 and 1 pairs-out).  By source form: VAR_DIRECT on all six variants, VAR_MULTI on generic / lds / dma / k4 /
                   streamlds, VAR_POOL2 (pooled and sub-sampled) on generic and streamlds.
                   Refused (4): streamlds at tile_c 2 and 4 on the 16-wide pooled and sub-sampled slices — one half k-step, the kernel needs 2 (MAF_E_UNSUPPORTED, nothing written).
    OP_CONV3X3S2   generic 138 (+ 22 fp32, 32 twin), lds 87 (+ 20 twin), dma 102 (+ 20 twin), k4 52 (+ 12 twin, 8 fp32), ldsall (CONV3_LDS) 25 + 30 with the pooled branch,
                   wreg (CONV3_WREG) 36 + 36 twin + 24 with the pooled branch; none refused (the twin at 256 workgroups per conv, which the tuner does not list, runs too).
    OP_DWCONV      generic 55 cost-model + 110 explicit tiles (+ 3 + 6 fp32), dot2 165, matrix-core 28, pixel-pair 256 (32 on each of 1 .. 8 waves), pixel-pair staged 102.
                   Refused (474, all MAF_E_ARG by the staged form's own precondition, nothing written): every staged tile where the waves do not divide Cin / 8 (8, 24 and 72
                   channels: 1, 3 and 9 groups); 16 x 20 tiles everywhere (rows * columns / 4 = 80 > 64, next to 16 x 16 and 8 x 32 at exactly 64, which run); 4 x 8 tiles
                   everywhere and 8 x 16 under k = 3 (three cases; planes below 4160 bytes per wave, next to 12 x 16, which runs).
    OP_STEM        18 sliced + 18 dense-output launches: u8 / f16 / f32 images x f16 / f32 outputs.     OP_SPPF_POOL  LDS kernel 4, fallback 3 (one fp32 each).
    OP_BOTTLENECK  12 (c 8, 32, 40, 64) + 11 with the closing conv (all six instantiations, five of them also with a c below their maximum: 8, 16, 40, 40, 56) + 66 bit-identical
                   launches on two streams.     OP_CONV1DW  9 (c 8, 72, 192).
    OP_STEM2       18: the three channel pairs with and without the third conv, the split second output, rows 4 and 8, u8 / f16 / f32 images.
    OP_HEADTAIL    20: widths 64 .. 384 x 1, 15, 17, 65 pixels per image, iters 0 / 1 / 3.
Largest err / bound seen per entry point (family B and the pooled branches; the bound is op_ref's, these are only what it left unused):
    OP_CONV1X1 generic 0.202, lds 0.195, dma 0.195, k4 0.195, stream 0.038, streamlds 0.202        OP_CONV3X3S2 generic / lds / dma / k4 0.200, ldsall 0.173 (pooled branch 0.196),
    wreg 0.171 (pooled branch 0.203)        OP_DWCONV generic 0.235, dot2 0.235, matrix-core 0.231, pixel-pair 0.235, staged 0.222        OP_STEM (u8) 0.167
    OP_CONV1DW 0.156        OP_BOTTLENECK 0.045, with the closing conv 0.036        OP_STEM2 0.018, with the third conv 0.003        OP_HEADTAIL 0.004
Every family-E case passed bit for bit, every family-B case inside the bound, no sentinel was touched and no NaN neighbour was read: nothing had to be fixed.
Wall time of the file on the MI355X: 3.9 s (276 tests).
"""
import ctypes as C
import functools

import pytest
import torch

from maf_yolo_amd import conv_variants, lib, pack

import fwd_ref as R
import op_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
SENT = 12344.0                  # (a multiple of 8: the same number in fp16 and fp32; above every input, so a max-pool that reads it shows it)
BIG = 2.0 ** 15                 # finite poison of a source read through a maximum
NAN = float("nan")
_TDT = {"f16": F16, "f32": F32, "u8": torch.uint8}
_LDT = {"f16": lib.F16, "f32": lib.F32, "u8": lib.U8}
TALLY = {}                      # (op, variant) -> [accepted, [refused (case, tile, error)]]
WORST = {}                      # entry point -> largest err / bound of family B


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(op):
    """None, or the library's error text for a refusal."""
    rc = lib.load().maf_op_launch(C.byref(op), _stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                  # a fault of the device: nothing more is started on it
        pytest.exit("the device reported %s after a launch of kind %d, tiles %s: stopping" % (e, op.kind, (op.tile_p, op.tile_c, op.tile_k)), returncode=3)
    if rc == -3:                                               # MAF_E_HIP: the runtime turned the launch down — not a refusal of the library
        pytest.fail("HIP error from a launch of kind %d, tiles %s: %s" % (op.kind, (op.tile_p, op.tile_c, op.tile_k), lib.load().maf_last_error().decode()))
    return None if rc == 0 else "%d: %s" % (rc, lib.load().maf_last_error().decode())


def _round8(n):
    return -(-n // 8) * 8


class _Src:
    """t [B, H, W, C] as the channel slice [coff, coff + C) of a buffer of pixel stride C + pad: the other channels, and one pixel before and after, hold `poison`.
    pairs: the whole buffer in the pixel-pair layout (one pair of poison before and after)."""

    def __init__(self, t, pad, front, poison=NAN, pairs=False):
        B, H, W, Cc = t.shape
        npix = B * H * W
        self.stride, self.coff = Cc + pad, pad if front else 0
        wide = torch.full((npix, self.stride), poison, dtype=t.dtype, device=DEV)
        wide[:, self.coff:self.coff + Cc] = t.reshape(npix, Cc).to(DEV)
        if pairs:
            body = pack.pairs_from_nhwc(wide.view(B, H, W, self.stride)).reshape(npix // 2, self.stride, 2)
            self.buf = torch.full((npix // 2 + 2, self.stride, 2), poison, dtype=t.dtype, device=DEV)
        else:
            body = wide
            self.buf = torch.full((npix + 2, self.stride), poison, dtype=t.dtype, device=DEV)
        self.buf[1:-1] = body
        self.ptr = self.buf[1].data_ptr()                     # pixel 0, channel 0 of the wide buffer

    def put(self, s, C_, mode):
        s.ptr, s.C, s.stride, s.coff, s.mode = self.ptr, C_, self.stride, self.coff, mode


class _Out:
    """[B, H, W] pixels of pixel stride `stride`, one more pixel before and after: NaN in the slices [(coff, C), ...], the sentinel elsewhere."""

    def __init__(self, bhw, dtype, slices, stride, pairs=False):
        self.bhw, self.slices, self.stride, self.pairs = tuple(bhw), slices, stride, pairs
        npix = bhw[0] * bhw[1] * bhw[2]
        self.buf = torch.full((npix // 2 + 2, stride, 2) if pairs else (npix + 2, stride), SENT, dtype=dtype, device=DEV)
        for o, n in slices:
            self.buf[1:-1, o:o + n] = NAN
        self.ptr = self.buf[1].data_ptr()

    def _nhwc(self):
        B, H, W = self.bhw
        if self.pairs:
            return self.buf[1:-1].reshape(B, H, W // 2, self.stride, 2).transpose(3, 4).reshape(B, H, W, self.stride)
        return self.buf[1:-1].reshape(B, H, W, self.stride)

    def got(self, i=0):
        o, n = self.slices[i]
        return self._nhwc()[..., o:o + n]

    def assert_rest_untouched(self, tag):
        b = self.buf.clone()
        for o, n in self.slices:
            b[1:-1, o:o + n] = SENT
        assert bool((b == SENT).all()), "%s: wrote outside its slice (%d elements)" % (tag, int((b != SENT).sum()))

    def assert_unwritten(self, tag):
        self.assert_rest_untouched(tag)
        for o, n in self.slices:
            s = self.buf[1:-1, o:o + n]
            assert bool((s != s).all()), "%s: a refused launch wrote to its output" % tag


def _assert_exact(got, want, tag):
    if torch.equal(got, want):
        return
    d = got.double() - want.double()
    bad = ~(d == 0)
    fin = ~torch.isnan(d)
    pytest.fail("%s: %d of %d elements differ (%d NaN); max |diff| %s; first (index, got, want): %s" % (
        tag, int(bad.sum()), bad.numel(), int((~fin).sum()), float(d[fin].abs().max()) if bool(fin.any()) else None,
        [(i, float(got[tuple(i)]), float(want[tuple(i)])) for i in bad.nonzero()[:12].tolist()]))


@functools.lru_cache(maxsize=None)
def _ref(name):
    return {k: tuple(None if t is None else t.to(DEV) for t in v) for k, v in R.case_reference(R.BY_NAME[name]).items()}


def _check(c, key, got, tag, entry):
    ref, bnd, _ = _ref(c["name"])[key]
    if R.is_exact(c, key):
        _assert_exact(got, ref.to(got.dtype), tag + " " + key)
        return
    err = (got.double() - ref).abs()
    ratio = float((err / bnd).max())
    ratio = ratio if ratio == ratio else float("inf")
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    assert bool((err <= bnd).all()), "%s %s %s: err / bound %.4f (%d NaN)" % (entry, tag, key, ratio, int(torch.isnan(err).sum()))


def _count(op, variant, refused=None):
    t = TALLY.setdefault((op, variant), [0, []])
    if refused is None:
        t[0] += 1
    else:
        t[1].append(refused)


def _dev(t):
    return t.to(DEV)


# --------------------------------------------------------------------------------------------------------------------------------- OP_CONV1X1 / OP_CONV3X3S2
def _conv_tiles(c):
    kind = lib.OP_CONV3X3S2 if c["kind"] == "conv3" else lib.OP_CONV1X1
    H, W = R.out_grid(c)
    out = []
    for M in (c["B"] * H * W, 65536):
        out += conv_variants.conv_tiles(kind, _LDT[c["dtype"]], M, c["srcs"], c["cout"], 8, bool(c.get("out_f32")), bool(c.get("twin")))
    out += c.get("extra", [])
    return [t for t in dict.fromkeys(out) if not c.get("only") or t[2] in c["only"]]


def _poison(mode):
    return BIG if mode == R.POOL2 else NAN


def _conv_sources(c, o, flip):
    """The sources of one conv of the case (o: its operands), each in a poisoned buffer of its own; the slice at the front / the back in turn."""
    modes = [m for _, m in c["srcs"]]
    return [_Src(t, 8 * (1 + (i + flip) % 2), bool((i + flip + len(c["name"])) % 2), _poison(m)) for i, (t, m) in enumerate(zip(o["srcs"], modes))]


def _conv_weights(c, o, tile, cache, pool1=None):
    pt, ct, tk = tile
    dt = _LDT[c["dtype"]]
    key = (id(o), ct if tk not in (lib.CONV3_LDS, lib.CONV3_WREG) else -tk, pool1 is not None)
    if key not in cache:
        w, b = o["w"], o["b"]
        if tk == lib.CONV3_LDS:
            cache[key] = (_dev(pack.pack_mprep_lds(w, b, *pool1) if pool1 else pack.pack_conv3x3_lds(w, b)), _dev(pack.pack_bias(b, 4)))
        elif tk == lib.CONV3_WREG:
            cache[key] = (_dev(pack.pack_mprep_wreg(w, b, *pool1) if pool1 else pack.pack_conv3x3_wreg(w, b)), _dev(pack.pack_bias(b, 4)))
        elif c["kind"] == "conv3":
            cache[key] = (_dev(pack.pack_conv3x3(w, ct, dt)), _dev(pack.pack_bias(b, ct)))
        else:
            cache[key] = (_dev(pack.pack_conv1x1(w, [s[0] for s in c["srcs"]], ct, dt)), _dev(pack.pack_bias(b, ct)))
    return cache[key]


@functools.lru_cache(maxsize=None)
def _run_conv_case(name):
    """Every candidate of the case; returns (ran, refused)."""
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    opname = "OP_CONV3X3S2" if c["kind"] == "conv3" else "OP_CONV1X1"
    H, W = R.out_grid(c)
    B, cout, nc = c["B"], c["cout"], c.get("nc", 0)
    tdt = R.store_dtype(c)
    srcs = _conv_sources(c, inp, 0)
    tsrcs = _conv_sources(c, inp["twin"], 0) if c.get("twin") else None              # (same stride and offset as the first conv's: the twin shares them)
    cache, ran, refused = {}, [], []
    pairs = bool(c.get("out_pairs"))
    for tile in _conv_tiles(c):
        pt, ct, tk = tile
        fused = tk in (lib.CONV3_LDS, lib.CONV3_WREG)
        if nc and c["pool_front"]:
            slices = [(8 + nc, cout), (8, nc)]
        elif nc:
            slices = [(8, cout), (8 + cout, nc)]
        else:
            slices = [(8 if len(ran) % 2 == 0 else 0, cout)]                          # the output slice at the front / the back in turn
        stride = _round8(8 + cout + nc + 8)
        outs = [_Out((B, H, W), tdt, slices, stride, pairs)] + ([_Out((B, H, W), tdt, slices, stride)] if tsrcs else [])
        wp, bp = _conv_weights(c, inp, tile, cache, inp.get("pool1") if nc else None)
        op = lib.MafOp()
        op.kind, op.dtype, op.in_dtype, op.act = (lib.OP_CONV3X3S2 if c["kind"] == "conv3" else lib.OP_CONV1X1), _LDT[c["dtype"]], _LDT[c["dtype"]], c["act"]
        op.B, op.H, op.W, op.Hin, op.Win, op.Cin, op.Cout, op.nsrc = B, H, W, c.get("Hin", 0), c.get("Win", 0), sum(s[0] for s in c["srcs"]), cout, len(srcs)
        for i, (s, (C_, m)) in enumerate(zip(srcs, c["srcs"])):
            s.put(op.src[i], C_, m)
        op.out, op.out_stride, op.out_coff = outs[0].ptr, stride, slices[0][0]
        op.out_f32, op.out_pairs = int(bool(c.get("out_f32"))), int(pairs)
        op.tile_p, op.tile_c, op.tile_k = pt, ct, tk
        op.w, op.bias = wp.data_ptr(), bp.data_ptr()
        if nc:
            op.nc, op.reg_stride = nc, slices[1][0]
        if tsrcs:
            wp2, bp2 = _conv_weights(c, inp["twin"], tile, cache)
            op.aux[0], op.aux[1], op.aux[2], op.aux[3] = tsrcs[0].ptr, wp2.data_ptr(), bp2.data_ptr(), outs[1].ptr
        variant = lib.CONV_VARIANT_NAMES[tk] + (" tile_p 2" if tk == lib.CONV_STREAM_LDS and pt == 2 else "") + (" twin" if tsrcs else "") + (" pooled" if nc else "") + \
            (" pairs-out" if pairs else "") + (" f32-out" if c.get("out_f32") else "") + (" fp32" if c["dtype"] == "f32" else "")
        var = "VAR_3X3S2" if c["kind"] == "conv3" else "VAR_MULTI" if len(srcs) > 1 else "VAR_POOL2" if c["srcs"][0][1] in (R.POOL2, R.SUB2) else "VAR_DIRECT"
        tag = "%s %s" % (name, tile)
        err = _launch(op)
        if err is not None:
            for o in outs:
                o.assert_unwritten(tag + " (refused: %s)" % err)
            refused.append((tile, err))
            _count(opname, variant, (name, tile, err))
            continue
        for o, key in zip(outs, ("out", "twin")):
            o.assert_rest_untouched(tag + " " + key)
            _check(c, key, o.got(0), tag, "%s %s" % (opname, lib.CONV_VARIANT_NAMES[tk]))
            if nc:
                _check(c, "pool", o.got(1), tag, "%s %s pooled branch" % (opname, lib.CONV_VARIANT_NAMES[tk]))
        ran.append(tile)
        _count(opname, variant)
        _count(opname, var + " " + lib.CONV_VARIANT_NAMES[tk])
    return ran, refused


@pytest.mark.parametrize("name", R.names("conv1"))
def test_conv1x1_on_every_candidate(name):
    ran, refused = _run_conv_case(name)
    print("conv1x1 %s: %d candidates ran, refused: %s" % (name, len(ran), refused))
    assert ran, "%s: every candidate was refused: %s" % (name, refused)


@pytest.mark.parametrize("name", R.names("conv3"))
def test_conv3x3s2_on_every_candidate(name):
    ran, refused = _run_conv_case(name)
    print("conv3x3s2 %s: %d candidates ran, refused: %s" % (name, len(ran), refused))
    assert ran, "%s: every candidate was refused: %s" % (name, refused)


# -------------------------------------------------------------------------------------------------------------------------------------------------- OP_DWCONV
def _dw_variants(c):
    """(variant, tile_p, tile_c, tile_k) of every launch of a depth-wise case."""
    H, W, Cc, k = c["H"], c["W"], c["C"], c["k"]
    cout = Cc * (2 if c["two"] else 1)
    n = 8 if c["dtype"] == "f16" else 4
    v = [("generic cost-model", 0, 0, 0),
         ("generic explicit", 4, 8, 2 * n),                             # 16 (8) channels per block: a partial last block at 8, 24, 72 (12) channels
         ("generic explicit", 3, 4, 5 * n)]                             # 3 rows x 4 columns x 40 (20) channels: ragged on every axis
    if c["dtype"] != "f16":
        return v
    w8 = _round8(W)
    v += [("dot2 tile wider than the map", lib.DW_DOT2, w8 + 8, (H + 1) * 256 + 8),
          ("dot2 partial last tile on both axes", lib.DW_DOT2, 8, 2 * 256 + 16),
          ("dot2", lib.DW_DOT2, 16, 5 * 256 + 64)]
    if not c["two"]:
        v.append(("matrix-core", lib.DW_MFMA, 0, 0))
    if W % 2 == 0:
        for nw in range(1, 9):                                         # tile columns 4 (W = 2: wider than the map), else 8 (W = 4: wider; W = 20: a last tile of 4)
            v.append(("pixel-pair %d waves" % nw, lib.DW_PAIRS, 4 if W == 2 or nw % 2 else 8, (3 if nw % 3 else 4) * 256 + nw))
        # staged stores (dwconv_p2.hip): 2 / 4 / 8 waves dividing Cin / 8, rows * columns / 4 <= 64 (16 x 16 and 8 x 32: exactly 64; 16 x 20: 80, refused), planes of >= 4160
        # bytes per wave (4 x 8 under k = 3: refused)
        for th, tw in ((16, 16), (8, 32), (16, 20), (4, 8), (8, 16), (12, 16)):
            for nw in (2, 4, 8):
                v.append(("pixel-pair staged", lib.DW_PAIRS, tw, th * 256 + nw + lib.DW_P2_STAGED))
    return v


@functools.lru_cache(maxsize=None)
def _run_dw_case(name):
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    B, H, W, Cc, k = c["B"], c["H"], c["W"], c["C"], c["k"]
    cout = Cc * (2 if c["two"] else 1)
    tdt, dt = _TDT[c["dtype"]], _LDT[c["dtype"]]
    front = bool(len(name) % 2)
    src = _Src(inp["srcs"][0], 16, front)
    psrc = _Src(inp["srcs"][0], 8, not front, pairs=True) if W % 2 == 0 and c["dtype"] == "f16" else None
    wp, bp = _dev(pack.pack_dw(inp["w"], dt)), _dev(inp["b"])
    wpairs = _dev(pack.pack_dw_pairs(inp["w"])) if psrc else None
    toe = _dev(pack.pack_dw_toeplitz(inp["w"])) if c["dtype"] == "f16" and not c["two"] else None
    ran, refused = [], []
    for variant, tp, tc, tk in _dw_variants(c):
        stride = _round8(cout + 24)
        out = _Out((B, H, W), tdt, [(8 if len(ran) % 2 == 0 else 16, cout)], stride)
        op = lib.MafOp()
        op.kind, op.dtype, op.in_dtype, op.act = lib.OP_DWCONV, dt, dt, c["act"]
        op.B, op.H, op.W, op.Cin, op.Cout, op.ksize, op.nsrc = B, H, W, Cc, cout, k, 1
        (psrc if tp == lib.DW_PAIRS else src).put(op.src[0], Cc, lib.SRC_PAIRS if tp == lib.DW_PAIRS else lib.SRC_DIRECT)
        op.out, op.out_stride, op.out_coff = out.ptr, stride, out.slices[0][0]
        op.tile_p, op.tile_c, op.tile_k = tp, tc, tk
        op.w, op.bias = wp.data_ptr(), bp.data_ptr()
        if tp == lib.DW_PAIRS:
            op.aux[1] = wpairs.data_ptr()
        if tp == lib.DW_MFMA:
            op.aux[0] = toe.data_ptr()
        tag = "%s %s %s" % (name, variant, (tp, tc, tk))
        fam = variant.split(" tile")[0].split(" partial")[0] if variant.startswith("dot2") else "pixel-pair" if variant.startswith("pixel-pair ") and "staged" not in variant else variant
        err = _launch(op)
        if err is not None:
            out.assert_unwritten(tag + " (refused: %s)" % err)
            refused.append(((tp, tc, tk), err))
            _count("OP_DWCONV", fam, (name, (tp, tc, tk), err))
            continue
        out.assert_rest_untouched(tag)
        _check(c, "out", out.got(0), tag, "OP_DWCONV " + fam)
        ran.append((tp, tc, tk))
        _count("OP_DWCONV", fam + (" fp32" if c["dtype"] == "f32" else ""))
        if variant.endswith(" waves"):
            _count("OP_DWCONV", variant)
    return ran, refused


@pytest.mark.parametrize("name", R.names("dw"))
def test_depthwise_on_every_kernel(name):
    c = R.BY_NAME[name]
    ran, refused = _run_dw_case(name)
    print("dwconv %s: %d launches ran, refused: %s" % (name, len(ran), refused))
    assert (0, 0, 0) in ran and len([t for t in ran if t[0] > 0]) == 2, "the generic kernel takes every case: %s" % (refused,)
    if c["dtype"] == "f16":
        assert len([t for t in ran if t[0] == lib.DW_DOT2]) == 3 and (c["two"] or (lib.DW_MFMA, 0, 0) in ran), refused
        if c["W"] % 2 == 0:
            assert len([t for t in ran if t[0] == lib.DW_PAIRS and not t[2] & lib.DW_P2_STAGED]) == 8, refused


# ---------------------------------------------------------------------------------------------------------------------------------------------------- OP_STEM
@pytest.mark.parametrize("name", R.names("stem"))
def test_stem(name):
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    B, Hin, Win, cout = c["B"], c["Hin"], c["Win"], c["cout"]
    H, W = R.out_grid(c)
    img = inp["image"]
    buf = torch.full((img.numel() + 32,), 255 if c["in_dtype"] == "u8" else NAN, dtype=img.dtype, device=DEV)      # 16 poisoned elements before and after the image
    buf[16:-16] = img.reshape(-1).to(DEV)
    stride = cout + 16
    out = _Out((B, H, W), _TDT[c["dtype"]], [(8 if len(name) % 2 else 0, cout)], stride)
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype, op.act = lib.OP_STEM, _LDT[c["dtype"]], _LDT[c["in_dtype"]], lib.ACT_RELU
    op.B, op.H, op.W, op.Hin, op.Win, op.Cin, op.Cout, op.nsrc = B, H, W, Hin, Win, 3, cout, 1
    op.src[0].ptr = buf[16:].data_ptr()
    op.out, op.out_stride, op.out_coff = out.ptr, stride, out.slices[0][0]
    ws, bs = _dev(pack.pack_stem(inp["w"])), _dev(inp["b"])
    op.w, op.bias = ws.data_ptr(), bs.data_ptr()
    err = _launch(op)
    assert err is None, err
    out.assert_rest_untouched(name)
    _check(c, "out", out.got(0), name, "OP_STEM %s image" % c["in_dtype"])
    _count("OP_STEM", "%s image, %s output" % (c["in_dtype"], c["dtype"]))
    dense = _Out((B, H, W), _TDT[c["dtype"]], [(0, cout)], cout)          # a dense output: the form that leaves through LDS (the pixel before and after: sentinel)
    op.out, op.out_stride, op.out_coff = dense.ptr, cout, 0
    err = _launch(op)
    assert err is None, err
    dense.assert_rest_untouched(name + " dense")
    _check(c, "out", dense.got(0), name + " dense", "OP_STEM %s image" % c["in_dtype"])
    _count("OP_STEM", "dense output")


# --------------------------------------------------------------------------------------------------------------------------------------------------- OP_STEM2
@pytest.mark.parametrize("name", R.names("stem2"))
def test_stem2(name):
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    B, Hin, Win, C0, C1 = c["B"], c["Hin"], c["Win"], c["C0"], c["cout"]
    H, W = R.out_grid(c)
    img, raw = inp["image"], inp["raw"]
    buf = torch.full((img.numel() + 32,), 255 if c["in_dtype"] == "u8" else NAN, dtype=img.dtype, device=DEV)      # 16 poisoned elements before and after the image
    buf[16:-16] = img.reshape(-1).to(DEV)
    rec = _dev(pack.pack_stem2(*raw))
    assert rec.numel() == lib.load().maf_stem2_record_bytes(C0, C1, C1 if c["third"] else 0)
    wout = C1 // 2 if c["split"] else C1
    out = _Out((B, H, W), F16, [(16 if len(name) % 2 else 8, wout)], _round8(wout + 24))
    out2 = _Out((B, H, W), F16, [(8, wout)], wout + 16) if c["split"] else None
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype, op.act = lib.OP_STEM2, lib.F16, _LDT[c["in_dtype"]], lib.ACT_RELU
    op.B, op.H, op.W, op.Hin, op.Win, op.Cin, op.Cout, op.ksize, op.nsrc = B, H, W, Hin, Win, 3, C1, C0, 1
    op.nc = C1 if c["third"] else 0
    op.src[0].ptr, op.src[0].C = buf[16:].data_ptr(), 3
    op.out, op.out_stride, op.out_coff = out.ptr, out.stride, out.slices[0][0]
    op.tile_p, op.tile_k = c["rows"], 0
    op.w = rec.data_ptr()
    if out2 is not None:
        op.aux[0], op.reg_stride = out2.buf[1, 8:].data_ptr(), out2.stride            # (a tensor of its own: the pointer is its channel 0)
    err = _launch(op)
    assert err is None, err
    entry = "OP_STEM2" + (" with the third conv" if c["third"] else "")
    for o, key in ((out, "out"), (out2, "out2")):
        if o is not None:
            o.assert_rest_untouched(name + " " + key)
            _check(c, key, o.got(0), name, entry)
    _count("OP_STEM2", "%d -> %d%s%s" % (C0, C1, ", third conv" if c["third"] else "", ", split" if c["split"] else ""))
    _count("OP_STEM2", "%s image" % c["in_dtype"])
    _count("OP_STEM2", "rows %d" % c["rows"])


# ------------------------------------------------------------------------------------------------------------------------------------------------ OP_HEADTAIL
@pytest.mark.parametrize("name", R.names("head"))
def test_head_tail_writes_its_level_s_rows_alone(name):
    """The level's H W rows in the middle of a larger prediction [B, A, 85] (fp32): NaN before the launch, the rows of the other levels around them hold the sentinel."""
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    B, H, W, cc = c["B"], c["H"], c["W"], c["c"]
    srcs = [_Src(t, 8 * (1 + i), bool((i + len(name)) % 2)) for i, t in enumerate(inp["srcs"])]
    A = R.HEAD_BEFORE + H * W + R.HEAD_AFTER
    pred = torch.full((B, A, 85), SENT, dtype=F32, device=DEV)
    pred[:, R.HEAD_BEFORE:R.HEAD_BEFORE + H * W] = NAN
    recs = [_dev(pack.pack_head_tail(*inp["raw"][4 * i:4 * i + 4])) for i in range(2)]
    assert recs[0].numel() == lib.load().maf_head_tail_record_bytes(cc)
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype = lib.OP_HEADTAIL, lib.F16, lib.F16
    op.B, op.H, op.W, op.Cin, op.Cout, op.nsrc = B, H, W, cc, 85, 2
    for i, s_ in enumerate(srcs):
        s_.put(op.src[i], cc, lib.SRC_DIRECT)
    op.w, op.aux[0] = recs[0].data_ptr(), recs[1].data_ptr()
    op.out = pred.data_ptr()
    op.Hin, op.Win = R.HEAD_BEFORE, A
    op.lvl_stride[0], op.nc, op.reg_max = float(c["stride"]), 80, 16
    op.tile_k = c["iters"]
    err = _launch(op)
    assert err is None, err
    rest = pred.clone()
    rest[:, R.HEAD_BEFORE:R.HEAD_BEFORE + H * W] = SENT
    assert bool((rest == SENT).all()), "%s: wrote to the rows of another level" % name
    _check(c, "out", pred[:, R.HEAD_BEFORE:R.HEAD_BEFORE + H * W], name, "OP_HEADTAIL")
    _count("OP_HEADTAIL", "width %d" % cc)
    _count("OP_HEADTAIL", "iters %d" % c["iters"])


# ----------------------------------------------------------------------------------------------------------------------------------------------- OP_SPPF_POOL
@pytest.mark.parametrize("name", R.names("sppf"))
def test_sppf_pool_in_place_in_the_concat_buffer(name):
    """Source and outputs are slices of ONE buffer, as in the engine: x in [8, 8 + C), the three pools behind it (NaN before the launch), the sentinel — above every
    input, so that a maximum that reads it shows it — in the other channels and in the pixel before and after."""
    c = R.BY_NAME[name]
    x = R.inputs(c)["srcs"][0]
    B, H, W, Cc = x.shape
    stride = 8 + 4 * Cc + 8
    out = _Out((B, H, W), _TDT[c["dtype"]], [(8 + Cc, 3 * Cc), (8, Cc)], stride)
    out.buf[1:-1, 8:8 + Cc] = x.reshape(-1, Cc).to(DEV)
    op = lib.MafOp()
    op.kind, op.dtype, op.B, op.H, op.W, op.nsrc = lib.OP_SPPF_POOL, _LDT[c["dtype"]], B, H, W, 1
    op.src[0].ptr, op.src[0].C, op.src[0].stride, op.src[0].coff, op.src[0].mode = out.ptr, Cc, stride, 8, lib.SRC_DIRECT
    op.out, op.out_stride, op.out_coff = out.ptr, stride, 8 + Cc
    err = _launch(op)
    assert err is None, err
    out.assert_rest_untouched(name)
    assert torch.equal(out.got(1), x.to(DEV)), "the source slice changed"
    _check(c, "out", out.got(0), name, "OP_SPPF_POOL")
    _count("OP_SPPF_POOL", ("LDS kernel" if H <= 64 and W <= 64 else "fallback") + (" fp32" if c["dtype"] == "f32" else ""))


# ------------------------------------------------------------------------------------------------------------------------------ OP_BOTTLENECK / OP_CONV1DW
FINITE_POISON = {}              # fused case -> why its source poison is the largest finite fp16 value and not NaN (none needed it)


def _fused_op(c, srcs, out):
    """(op, keep-alive) of a fused case on the given sources and output."""
    inp = R.inputs(c)
    raw, k, cc = inp["raw"], c["k"], c["c"]
    op = lib.MafOp()
    op.dtype, op.in_dtype, op.act = lib.F16, lib.F16, lib.ACT_SILU
    op.B, op.H, op.W, op.Cin, op.ksize, op.nsrc = c["B"], c["H"], c["W"], cc, k, len(srcs)
    for i, s in enumerate(srcs):
        s.put(op.src[i], cc, lib.SRC_DIRECT)
    op.out, op.out_stride, op.out_coff = out.ptr, out.stride, out.slices[0][0]
    if c["sub"] == "c1dw":
        rec, nmb = pack.pack_conv1dw(raw[0], raw[1], inp["w"], raw[3])
        assert rec.shape[1] == lib.load().maf_conv1dw_record_bytes(k, cc)
        keep = [_dev(rec)]
        op.kind, op.Cout, op.w = lib.OP_CONV1DW, 3 * cc, keep[0].data_ptr()
        return op, keep
    rec, b2p, nmb, ct2 = pack.pack_bottleneck(raw[0], raw[1], inp["w"], raw[3], raw[4], raw[5])
    assert rec.shape[1] == lib.load().maf_bottleneck_record_bytes(k, cc, cc)
    keep = [_dev(rec), _dev(b2p)]
    op.kind, op.Cout = lib.OP_BOTTLENECK, cc
    op.tile_p, op.tile_c, op.tile_k = 16, 16, nmb
    op.w, op.bias = keep[0].data_ptr(), keep[1].data_ptr()
    if c["sub"] == "tail":
        assert lib.load().maf_bottleneck_tail_supported(k, cc, len(srcs), c["c3"]) == 1
        rec3 = pack.pack_bottleneck_tail(raw[6], raw[7], cc, len(srcs))
        assert rec3.numel() == lib.load().maf_bottleneck_tail_record_bytes(cc, len(srcs), c["c3"])
        keep.append(_dev(rec3))
        op.nc, op.aux[0] = c["c3"], keep[2].data_ptr()
    return op, keep


def _fused_width(c):
    return {"c1dw": 3 * c["c"], "bneck": c["c"], "tail": c.get("c3", 0)}[c["sub"]]


@pytest.mark.parametrize("name", R.names("fused"))
def test_fused_bottleneck_and_conv1dw(name):
    c = R.BY_NAME[name]
    inp = R.inputs(c)
    poison = 65504.0 if name in FINITE_POISON else NAN
    srcs = [_Src(t, 8 * (1 + i % 2), bool((i + len(name)) % 2), poison) for i, t in enumerate(inp["srcs"])]
    wout = _fused_width(c)
    out = _Out((c["B"], c["H"], c["W"]), F16, [(8 if len(name) % 2 else 16, wout)], _round8(wout + 24))
    op, keep = _fused_op(c, srcs, out)
    err = _launch(op)
    assert err is None, err
    out.assert_rest_untouched(name)
    entry = {"c1dw": "OP_CONV1DW", "bneck": "OP_BOTTLENECK", "tail": "OP_BOTTLENECK with the closing conv"}[c["sub"]]
    _check(c, "out", out.got(0), name, entry)
    _count(entry, "c %d" % c["c"])


def test_bottleneck_66_launches_on_two_streams_are_bit_identical():
    """The smallest bottleneck case 66 times, alternating two streams: every result bit-identical to the first (the round-robin counter sets of the kernel and their
    re-arming)."""
    c = R.BY_NAME[R.names("fused", lambda c_: c_["sub"] == "bneck")[0]]
    inp = R.inputs(c)
    srcs = [_Src(inp["srcs"][0], 8, True)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, keeps = [], []
    torch.cuda.synchronize()
    for i in range(66):
        out = _Out((c["B"], c["H"], c["W"]), F16, [(8, c["c"])], _round8(c["c"] + 24))
        op, keep = _fused_op(c, srcs, out)
        torch.cuda.synchronize() if i == 0 else None
        rc = lib.load().maf_op_launch(C.byref(op), streams[i % 2].cuda_stream)
        assert rc == 0, lib.load().maf_last_error().decode()
        outs.append(out)
        keeps.append(keep)
    torch.cuda.synchronize()
    _check(c, "out", outs[0].got(0), c["name"], "OP_BOTTLENECK")
    for i, o in enumerate(outs):
        o.assert_rest_untouched("launch %d" % i)
        assert torch.equal(o.buf, outs[0].buf), "launch %d differs from launch 0" % i
    _count("OP_BOTTLENECK", "66 launches on two streams")


# ------------------------------------------------------------------------------------------------------------------------------------------------- the tally
NEED = {"OP_CONV1X1": ["generic", "generic fp32", "generic twin", "generic f32-out", "lds", "lds twin", "dma", "dma twin", "k4", "k4 twin", "k4 f32-out", "stream", "streamlds", "streamlds tile_p 2",
                       "streamlds pairs-out", "streamlds tile_p 2 pairs-out"] + ["%s %s" % (v, k) for v in ("VAR_DIRECT", "VAR_MULTI") for k in ("generic", "lds", "dma", "k4", "streamlds")] +
                      ["VAR_POOL2 generic", "VAR_POOL2 streamlds"],
        "OP_CONV3X3S2": ["generic", "generic fp32", "generic twin", "lds", "lds twin", "dma", "dma twin", "k4", "k4 twin", "ldsall", "ldsall pooled", "wreg", "wreg twin", "wreg pooled"],
        "OP_DWCONV": ["generic cost-model", "generic explicit", "generic cost-model fp32", "generic explicit fp32", "dot2", "matrix-core", "pixel-pair", "pixel-pair staged"] +
                     ["pixel-pair %d waves" % n for n in range(1, 9)],
        "OP_STEM": ["%s image, %s output" % (i, o) for i in ("u8", "f16", "f32") for o in ("f16", "f32")] + ["dense output"],
        "OP_SPPF_POOL": ["LDS kernel", "fallback", "LDS kernel fp32", "fallback fp32"],
        "OP_BOTTLENECK": ["c 8", "c 32", "c 40", "c 64", "66 launches on two streams"], "OP_BOTTLENECK with the closing conv": ["c %d" % n for n in (8, 16, 24, 32, 40, 48, 56, 64)],
        "OP_CONV1DW": ["c 8", "c 72", "c 192"],
        "OP_HEADTAIL": ["width %d" % w for w in (64, 128, 192, 256, 384)] + ["iters %d" % i for i in (0, 1, 3)],
        "OP_STEM2": ["%d -> %d%s" % (a, b, t) for a, b in R.STEM2_PAIRS for t in ("", ", third conv")] + ["u8 image", "f16 image", "f32 image", "rows 4", "rows 8"]}


def test_every_variant_family_ran_and_the_refusals_are_the_expected_ones():
    """Runs whatever case has not run yet (the per-case results are cached), then: every variant family above was accepted at least once per op, so refusals cannot
    hollow the suite out.  Prints the tally for the docstring."""
    for n in R.names("conv1") + R.names("conv3"):
        _run_conv_case(n)
    for n in R.names("dw"):
        _run_dw_case(n)
    for (op, variant), (n, refused) in sorted(TALLY.items()):
        print("TALLY %-14s %-36s accepted %4d  refused %3d %s" % (op, variant, n, len(refused), sorted({(r[1], r[2]) for r in refused})[:6]))
    for entry, r in sorted(WORST.items()):
        print("WORST %-44s %.4f" % (entry, r))
    for op, fams in NEED.items():
        if op not in ("OP_CONV1X1", "OP_CONV3X3S2", "OP_DWCONV") and not any(k[0] == op for k in TALLY):
            continue                                                  # (their tests keep no cache: run alone, this test has nothing to say about them)
        for f in fams:
            assert TALLY.get((op, f), [0])[0] > 0, "%s: no accepted launch of %r" % (op, f)
