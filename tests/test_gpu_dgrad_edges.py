"""-m gpu: the data-gradient kernels at their dispatch edges, straight through the C ABI, EXACTLY (references and cases: tests/dgrad_ref.py, checked by
test_dgrad_ref_host.py on the very tensors used here).

maf_op_launch with OP_CONV3X3S2_DGRAD (csrc/conv_mfma_dgrad.hip: the split parity-class form and the all-taps form of VAR_DGRAD3 on every one of its six tiles),
OP_CONV1X1 on a maf_pack_w1x1(transpose = 1) pack (every candidate train_ops.conv_candidates lists for the shape), OP_DWCONV on a maf_pack_dw(flip = 1) pack,
maf_dw_branches(dgrad = 1), maf_add_sub2, and the Python glue around them: _Conv1x1.backward (zero_padded / as_strided against F.pad), conv1x1s2, repvgg_convs,
_DWBranches.backward with an unused branch (autograd hands it a materialised zero dz; its `dy is None` branch cannot be reached that way and is not run).

dY is a channel slice of a wider buffer whose other channels, and the pixel before and after, are NaN: a read outside the slice poisons the result.  dX is written
into a slice of a wider buffer that holds NaN in the slice and a sentinel elsewhere; the sentinel must come back untouched.  Weights are packed from non-leaf tensors
(no staging-plan entry).  No MAF_* override is set: the branches are reached by shape, and dgrad_ref.CASES names, beside each case, the branch it is there for.

Family E (exact): integer inputs, zero bias, no activation — the fp32 accumulation is exact in any order and the one fp16 store of an integer <= 2048 is exact, so
torch.equal(got, ref.to(dtype)).  Family B (bound): wide_case inputs, n_terms <= 4096, per element |got - ref| <= ulp(ref) + K_CONV * n_terms * 2^-24 * S with the
storage type's ulp (the weight-gradient suite's derived bound + the one rounding of the store); the RepVGG sum: one more ulp of each addend (both are rounded to the
storage type before maf_add_sub2 adds them).

Largest err / bound seen per entry point (family B, MI355X; the bound is derived, these are only what it left unused — every one is below 0.5, the store's own
rounding of half an ulp: the accumulation term went unused):
    OP_CONV3X3S2_DGRAD             0.433   (all-taps form, 200 -> 72 on 2 x 5 x 7, n_terms 800; split form 0.380 at 384 -> 40, n_terms 1536; fp32 0.016; the same on all six tiles)
    OP_CONV1X1 (transposed pack)   0.495   (68 -> 192, n_terms 68; 0.449 at 576 -> 192; the same on every candidate, and with non-zero padding channels of dY)
    repvgg_convs backward          0.464   (24 <- 48 on 2 x 8 x 16, n_terms 192, with the two addends' ulps in the bound)
    OP_DWCONV (flipped pack)       0.492   (k 9, n_terms 81; fp32 0.099)
    maf_dw_branches (dgrad)        0.486   (k0 9, n_terms 130)
Family E per entry point: OP_CONV3X3S2_DGRAD (both forms, six tiles, fp16 and fp32; the tile_p = 4 entries of the tuner's list are refused cleanly),
OP_CONV1X1 on the transposed pack (11 .. 20 candidates per shape, none refused; at 192 -> 576 over 4551 pixels the generic kernel at tile_p 2 and 4 and
the LDS-shared-weight kernel at tile_p 2 among them), _Conv1x1.backward on both routes, conv1x1s2, repvgg_convs (the maf_stem_train
forward included), maf_add_sub2, OP_DWCONV on the flipped pack, maf_dw_branches(dgrad = 1) and _DWBranches.backward all passed untouched: nothing had to be fixed.
Wall time of the file on the MI355X: 4.1 s (150 tests).
"""
import contextlib
import ctypes as C

import pytest
import torch

from maf_yolo_amd import conv_variants, lib, pack, train_ops

import dgrad_ref as D
import op_ref
from wgrad_ref import conv_wgrad_ref, int_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
SENTINEL = -12344.0             # (a multiple of 8: the same number in fp16 and fp32)
_DT = {"f16": (F16, lib.F16), "f32": (F32, lib.F32)}
_REF = {}
_WORST = {}


def _ref(c):
    """The case's reference on the device, once: (dX, S, n_terms, parts)."""
    r = _REF.get(c["name"])
    if r is None:
        dx, S, n, parts = D.case_reference(c)
        parts = None if parts is None else tuple((a[0].to(DEV), a[1].to(DEV), a[2]) for a in parts)
        r = _REF[c["name"]] = (dx.to(DEV), S.to(DEV), n, parts)
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _embed(t, pad, front):
    """t [..., C] -> the same values as a channel slice of a buffer with pixel stride C + pad; the other channels, and one pixel before and after, are NaN."""
    Cc = t.shape[-1]
    npix = t.numel() // Cc
    buf = torch.full((npix + 2, Cc + pad), float("nan"), dtype=t.dtype, device=DEV)
    o = pad if front else 0
    buf[1:-1, o:o + Cc] = t.reshape(npix, Cc).to(DEV)
    return buf[1:-1].view(*t.shape[:-1], Cc + pad)[..., o:o + Cc]


def _nonleaf(w):
    """The weight on the device as a NON-LEAF tensor: train_ops' packers then pack here and now and make no staging-plan entry."""
    return w.to(DEV).requires_grad_(True) * 1


class _Out:
    """dX as a channel slice [coff, coff + C) of a buffer with pixel stride C + pad, one more pixel before and after: NaN in the slice, the sentinel elsewhere."""

    def __init__(self, shape, dtype, pad=16, coff=8):
        self.shape, self.C, self.coff = tuple(shape), shape[-1], coff
        npix = 1
        for d in shape[:-1]:
            npix *= d
        self.buf = torch.full((npix + 2, self.C + pad), SENTINEL, dtype=dtype, device=DEV)
        self.buf[1:-1, coff:coff + self.C] = float("nan")
        self.stride = self.C + pad
        self.ptr = self.buf[1].data_ptr()                     # pixel 0, channel 0 of the wide buffer: the slice starts out_coff channels in
        self.slice_ptr = self.buf[1, coff:].data_ptr()

    def got(self):
        return self.buf[1:-1, self.coff:self.coff + self.C].reshape(self.shape)

    def assert_rest_untouched(self, tag):
        b = self.buf.clone()
        b[1:-1, self.coff:self.coff + self.C] = SENTINEL
        assert bool((b == SENTINEL).all()), "%s: wrote outside its slice of dX (%d elements)" % (tag, int((b != SENTINEL).sum()))


def _assert_exact(got, want, tag):
    if torch.equal(got, want):
        return
    d = got.double() - want.double()
    bad = ~(d == 0)
    fin = ~torch.isnan(d)
    pytest.fail("%s: %d of %d elements differ (%d NaN); max |diff| %s; first (index, got - want): %s" % (
        tag, int(bad.sum()), bad.numel(), int((~fin).sum()), float(d[fin].abs().max()) if bool(fin.any()) else None,
        [(i, float(d[tuple(i)])) for i in bad.nonzero()[:12].tolist()]))


def _check(c, got, tag, entry, out=None, f32=None):
    """Family E: bit for bit; family B: the derived bound (its largest used fraction is printed and kept per entry point)."""
    dx, S, n, parts = _ref(c)
    f32 = c["dtype"] == "f32" if f32 is None else f32
    if out is not None:
        out.assert_rest_untouched(tag)
    if c["family"] == "E":
        _assert_exact(got, dx.to(got.dtype), tag)
        return
    assert n <= 4096
    bound = op_ref.ulp(dx, f32) + op_ref.K_CONV * n * 2.0 ** -24 * S
    if parts is not None:
        bound = bound + op_ref.ulp(parts[0][0], f32) + op_ref.ulp(parts[1][0], f32)
    err = (got.double() - dx).abs()
    ratio = float((err / bound).max())
    _WORST[entry] = max(_WORST.get(entry, 0.0), ratio)
    print("dgrad-B %s %s: n_terms %d, max err / bound %.4f (largest so far for the entry point %.4f)" % (entry, tag, n, ratio, _WORST[entry]))
    assert bool((err <= bound).all()), "%s %s: err / bound %.4f" % (entry, tag, ratio)


def _launch(op):
    """0, or the library's error text for a clean refusal."""
    rc = lib.load().maf_op_launch(C.byref(op), _stream())
    return None if rc == 0 else "%d: %s" % (rc, lib.load().maf_last_error().decode())


@contextlib.contextmanager
def _no_plan():
    """The autograd entry points run as a layer called without a Model does: no weight staging plan of an earlier test's model — and leave nothing behind: the tiles
    their tuners time and keep here (train_ops._conv_tune / _conv3_tune, process-wide, by shape) are dropped again, so no later test inherits a choice made on these
    tensors."""
    saved, train_ops._plan = train_ops._plan, None
    tunes = [(d, dict(d)) for d in (train_ops._conv_tune, train_ops._conv3_tune)]
    try:
        yield
    finally:
        train_ops._plan = saved
        for d, was in tunes:
            d.clear()
            d.update(was)


def _nchw(t):
    """An NHWC tensor (possibly a channel slice) as the [B, C, H, W] view autograd hands around."""
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ OP_CONV3X3S2_DGRAD (csrc/conv_mfma_dgrad.hip)
SIX = [(p, ct, 0) for p in (1, 2) for ct in (2, 4, 8)]


def _conv3_op(c, dy, wp_by_ct, tile, out, dt, w):
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    pt, ct, _ = tile
    if ct not in wp_by_ct:
        wp_by_ct[ct] = train_ops._packed_3x3(w, True, dt, ct, DEV)
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype, op.act = lib.OP_CONV3X3S2_DGRAD, dt, dt, lib.ACT_NONE
    op.B, op.H, op.W, op.Hin, op.Win, op.Cin, op.Cout, op.nsrc = B, H, W, dy.shape[1], dy.shape[2], cout, cin, 1
    op.src[0].ptr, op.src[0].C, op.src[0].stride, op.src[0].coff, op.src[0].mode = dy.data_ptr(), cout, dy.stride(2), 0, lib.SRC_DIRECT
    op.out, op.out_stride, op.out_coff = out.ptr, out.stride, out.coff
    op.tile_p, op.tile_c, op.tile_k = pt, ct, 0
    op.w, op.bias = wp_by_ct[ct].data_ptr(), train_ops._zero_bias(DEV, -(-cin // (16 * ct)) * 16 * ct).data_ptr()
    return op


@pytest.mark.parametrize("name", D.names("conv3"))
def test_conv3x3s2_dgrad_on_every_tile(name):
    """Every (tile_p, tile_c) conv_variants.conv3_dgrad_tiles offers for the shape — at its own pixel count and at one large enough for the list to hold its
    tile_p = 4 entries — and all six instantiations of the library whatever the list says.  A tile the library lacks is refused cleanly: exactly the tile_p = 4 ones."""
    c = D.BY_NAME[name]
    tdt, dt = _DT[c["dtype"]]
    inp = D.inputs(c)
    B, H, W, cin = c["B"], c["H"], c["W"], c["cin"]
    M = B * H * W
    static = (*train_ops._tile_dgrad(cin, M), 0)
    offered = conv_variants.conv3_dgrad_tiles(cin, M, static) + conv_variants.conv3_dgrad_tiles(cin, 1 << 22, static)
    tiles = list(dict.fromkeys(offered + SIX))
    assert any(t[0] == 4 for t in tiles) and set(SIX) <= set(tiles)
    dy = _embed(inp["dys"][0], 16, True)
    w = _nonleaf(inp["ws"][0])
    packs, refused, ran = {}, [], []
    for tile in tiles:
        out = _Out((B, H, W, cin), tdt)
        err = _launch(_conv3_op(c, dy, packs, tile, out, dt, w))
        torch.cuda.synchronize()
        if err is not None:
            refused.append(tile)
            assert bool((out.buf[1:-1, out.coff:out.coff + cin] != out.buf[1:-1, out.coff:out.coff + cin]).all()), "a refused launch wrote to dX"
            out.assert_rest_untouched("%s tile %s (refused: %s)" % (name, tile, err))
            continue
        ran.append(tile)
        _check(c, out.got(), "%s tile %s (%s form)" % (name, tile[:2], "split" if H % 2 == 0 and W % 2 == 0 else "all-taps"), "OP_CONV3X3S2_DGRAD", out)
    assert set(refused) == {t for t in tiles if t[0] == 4}, "refused %s of %s" % (refused, tiles)
    assert set(ran) >= set(SIX)


# --------------------------------------------------------------------------------------------------------------- OP_CONV1X1 on a transposed pack (1x1 data gradient)
def _conv1_op(c, dyk, kk, wp, tile, out, dt):
    B, H, W, cin = c["B"], c["H"], c["W"], c["cin"]
    pt, ct, tk = tile
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype, op.act = lib.OP_CONV1X1, dt, dt, lib.ACT_NONE
    op.B, op.H, op.W, op.Cin, op.Cout, op.nsrc = B, H, W, kk, cin, 1
    op.src[0].ptr, op.src[0].C, op.src[0].stride, op.src[0].coff, op.src[0].mode = dyk.data_ptr(), kk, dyk.stride(2), 0, lib.SRC_DIRECT
    op.out, op.out_stride, op.out_coff = out.ptr, out.stride, out.coff
    op.tile_p, op.tile_c, op.tile_k = pt, ct, tk
    op.w, op.bias = wp.data_ptr(), train_ops._zero_bias(DEV, -(-cin // (16 * ct)) * 16 * ct).data_ptr()
    return op


def _padded_dy(dy, kk, fill):
    """dY [B, H, W, cout] with its channels rounded up to kk, the padding channels holding `fill`."""
    if dy.shape[-1] == kk:
        return dy
    return torch.cat([dy, torch.full(dy.shape[:-1] + (kk - dy.shape[-1],), fill, dtype=dy.dtype)], -1)


def _conv1_run(c, cands):
    tdt, dt = _DT[c["dtype"]]
    inp = D.inputs(c)
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    mult = 8 if tdt == F16 else 4
    kk = -(-cout // mult) * mult
    w2d = _nonleaf(inp["ws"][0].reshape(cout, cin)).detach().contiguous()
    # padding channels of dY: zero as the producer leaves them, then NaN-free but non-zero — the packed weight rows there are zero, the result must not change
    dys = [_embed(_padded_dy(inp["dys"][0], kk, fill), 8, True) for fill in ((0.0, 5.0) if kk != cout else (0.0,))]
    packs, ran, refused = {}, [], []
    for tile in cands:
        ct = tile[1]
        if ct not in packs:
            packs[ct] = train_ops._packed_1x1(w2d, cout, cin, 1, dt, ct, DEV)
        for i, dyk in enumerate(dys):
            out = _Out((B, H, W, cin), tdt)
            err = _launch(_conv1_op(c, dyk, kk, packs[ct], tile, out, dt))
            torch.cuda.synchronize()
            if err is not None:
                refused.append((tile, err))
                out.assert_rest_untouched("%s %s (refused)" % (c["name"], tile))
                break
            _check(c, out.got(), "%s %s%s" % (c["name"], tile, " (padding channels of dY = 5)" if i else ""), "OP_CONV1X1 (transposed pack)", out)
        else:
            ran.append(tile)
    return ran, refused


@pytest.mark.parametrize("name", D.names("conv1", pred=lambda c: c["dtype"] == "f16" and "autograd" not in c["name"]))
def test_conv1x1_dgrad_on_every_candidate_of_the_training_tuner(name):
    c = D.BY_NAME[name]
    kk = -(-c["cout"] // 8) * 8
    cands = train_ops.conv_candidates(c["B"] * c["H"] * c["W"], kk, c["cin"])
    assert len(set(cands)) == len(cands)
    ran, refused = _conv1_run(c, cands)
    print("conv1x1 dgrad %s: %d candidates ran, refused: %s" % (name, len(ran), refused))
    assert len(ran) >= 6, "%s: only %d of %d candidates ran; refused: %s" % (name, len(ran), len(cands), refused)


@pytest.mark.parametrize("name", D.names("conv1", pred=lambda c: c["dtype"] == "f32"))
def test_conv1x1_dgrad_fp32_on_the_static_tile(name):
    c = D.BY_NAME[name]
    ran, refused = _conv1_run(c, [(*pack.tile_for(c["cin"], c["B"] * c["H"] * c["W"]), lib.CONV_GENERIC)])
    assert ran and not refused, refused


def test_conv1x1_backward_reads_a_registered_zero_padded_dy_in_place_and_pads_any_other():
    """_Conv1x1.backward with 68 output channels, twice: dY a 68-channel view of a 72-channel buffer registered in train_ops.zero_padded (read as 72 channels in
    place: no torch kernel), and the same view unregistered (F.pad).  Both exact, and equal."""
    c = D.BY_NAME["conv1-autograd-68"]
    inp = D.inputs(c)
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    g = torch.Generator().manual_seed(c["seed"])
    x0 = int_case((B, H, W, cin), g, n_terms=cin)
    wref = conv_wgrad_ref(x0, inp["dys"][0], 1, 1, exact=True)[0]
    got = []
    with _no_plan():
        for registered in (True, False):
            x = _nchw(x0.to(DEV)).requires_grad_(True)
            w = torch.nn.Parameter(inp["ws"][0].to(DEV))
            buf = torch.zeros(B, H, W, 72, dtype=F16, device=DEV)
            buf[..., :cout] = inp["dys"][0].to(DEV)
            dy = _nchw(buf)[:, :cout]
            y = train_ops.conv1x1(x, w)
            glue0 = train_ops.stats.get("glue", 0)
            try:
                if registered:
                    train_ops.zero_padded[buf.data_ptr()] = 72
                torch.autograd.backward([y], [dy])
                torch.cuda.synchronize()
            finally:
                train_ops.zero_padded.pop(buf.data_ptr(), None)
            assert (train_ops.stats.get("glue", 0) == glue0) == registered, "the %s route did not run" % ("as_strided" if registered else "F.pad")
            dx = x.grad.permute(0, 2, 3, 1)
            _check(c, dx, "conv1x1 backward, dY %s" % ("registered in zero_padded" if registered else "unregistered"), "_Conv1x1.backward")
            _assert_exact(w.grad.reshape(cout, cin), wref.to(DEV).float(), "conv1x1 backward: dW beside the checked dX")
            got.append(dx.clone())
    assert torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------------------------- 1x1 stride 2 and the RepVGG pair
def _x_for(c, g):
    """An integer input of the forward conv (its values do not reach dX); the image's channels 3..7 are zero."""
    x = int_case((c["B"], c["H"], c["W"], c["cin"]), g, n_terms=c["B"] * c["H"] * c["W"])
    x[..., c.get("cin_w", c["cin"]):] = 0
    return x


def _assert_dw(w, x0, dy, k, tag):
    """The weight gradient that ran beside the checked data gradient (csrc/wgrad.hip on the side stream): integers too, so exact."""
    ref = conv_wgrad_ref(x0, dy, k, 2, exact=True)[0].to(DEV).float()
    ref = ref.permute(2, 3, 0, 1) if k == 3 else ref.reshape(*ref.shape, 1, 1)
    _assert_exact(w.grad, ref[:, :w.shape[1]].contiguous(), tag)


@pytest.mark.parametrize("name", D.names("conv1s2"))
def test_conv1x1s2_backward_scatters_onto_the_even_pixels(name):
    c = D.BY_NAME[name]
    inp = D.inputs(c)
    x0 = _x_for(c, torch.Generator().manual_seed(c["seed"]))
    with _no_plan():
        x = _nchw(x0.to(DEV)).requires_grad_(True)
        w = torch.nn.Parameter(inp["ws"][0].to(DEV))
        y = train_ops.conv1x1s2(x, w)
        torch.autograd.backward([y], [_nchw(_embed(inp["dys"][0], 8, True))])
        torch.cuda.synchronize()
    dx = x.grad.permute(0, 2, 3, 1)
    _check(c, dx, name, "conv1x1s2 backward")
    odd = dx.clone()
    odd[:, ::2, ::2] = 0
    assert float(odd.abs().max()) == 0.0
    _assert_dw(w, x0, inp["dys"][0], 1, name + ": dW")


@pytest.mark.parametrize("name", D.names("repvgg"))
def test_repvgg_pair_backward_is_the_sum_of_its_two_gradients(name):
    """train_ops.repvgg_convs: the 3x3 stride-2 data gradient, the compact 1x1 stride-2 data gradient and maf_add_sub2 as the ONE gradient they produce."""
    c = D.BY_NAME[name]
    inp = D.inputs(c)
    x0 = _x_for(c, torch.Generator().manual_seed(c["seed"]))
    stem0 = train_ops.stats.get("native_stem_train", 0)
    with _no_plan():
        x = _nchw(x0.to(DEV)).requires_grad_(True)
        w3, w1 = torch.nn.Parameter(inp["ws"][0].to(DEV)), torch.nn.Parameter(inp["ws"][1].to(DEV))
        z3, z1 = train_ops.repvgg_convs(x, w3, w1)
        torch.autograd.backward([z3, z1], [_nchw(_embed(inp["dys"][0], 16, True)), _nchw(_embed(inp["dys"][1], 8, False))])
        torch.cuda.synchronize()
    assert (train_ops.stats.get("native_stem_train", 0) == stem0 + 1) == (c["cin_w"] == 3 and train_ops.stem_train)
    _check(c, x.grad.permute(0, 2, 3, 1), name, "repvgg_convs backward")
    if c["family"] == "E":
        _assert_dw(w3, x0, inp["dys"][0], 3, name + ": dW of the 3x3 branch")
        _assert_dw(w1, x0, inp["dys"][1], 1, name + ": dW of the 1x1 branch")


@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("name", ["repvgg-24to48-2x8x16", "repvgg-8to24-1x4x8"])
def test_add_sub2_joins_the_two_addends_in_place(name, dtype):
    """maf_add_sub2 on the reference's own addends: dst (the 3x3 gradient, a slice of a wider buffer) += src (the compact 1x1 gradient) on the even pixels only."""
    c = D.BY_NAME[name]
    dx, _, _, (a3, a1) = _ref(c)
    tdt, dt = _DT[dtype]
    B, H, W, cin = dx.shape
    out = _Out((B, H, W, cin), tdt)
    out.buf[1:-1, out.coff:out.coff + cin] = a3[0].to(tdt).reshape(-1, cin)
    src = _embed(a1[0][:, ::2, ::2].to(tdt).cpu(), 8, True)
    lib.check(lib.load().maf_add_sub2(src.data_ptr(), src.stride(2), out.slice_ptr, out.stride, B, H // 2, W // 2, cin, dt, _stream()))
    torch.cuda.synchronize()
    out.assert_rest_untouched(name)
    _assert_exact(out.got(), dx.to(tdt), "add_sub2 %s %s" % (name, dtype))


# ------------------------------------------------------------------------------------------------------------- OP_DWCONV on a flipped pack (csrc/dwconv.hip)
@pytest.mark.parametrize("name", D.names("dw"))
def test_depthwise_dgrad_is_the_forward_kernel_on_the_flipped_filter(name):
    c = D.BY_NAME[name]
    tdt, dt = _DT[c["dtype"]]
    inp = D.inputs(c)
    B, H, W, Cc, k = c["B"], c["H"], c["W"], c["C"], c["k"]
    dy = _embed(inp["dys"][0], 8, True)
    wp = train_ops._packed_dw(_nonleaf(inp["ws"][0]), Cc, k, 1, dt, DEV)
    out = _Out((B, H, W, Cc), tdt)
    op = lib.MafOp()
    op.kind, op.dtype, op.in_dtype, op.act = lib.OP_DWCONV, dt, dt, lib.ACT_NONE
    op.B, op.H, op.W, op.Cin, op.Cout, op.ksize, op.nsrc = B, H, W, Cc, Cc, k, 1
    op.src[0].ptr, op.src[0].C, op.src[0].stride, op.src[0].coff, op.src[0].mode = dy.data_ptr(), Cc, dy.stride(2), 0, lib.SRC_DIRECT
    op.out, op.out_stride, op.out_coff = out.ptr, out.stride, out.coff
    op.w, op.bias = wp.data_ptr(), train_ops._zero_bias(DEV, Cc).data_ptr()
    assert _launch(op) is None
    torch.cuda.synchronize()
    _check(c, out.got(), name, "OP_DWCONV (flipped pack)", out)


# ------------------------------------------------------------------------------------------------------------ maf_dw_branches(dgrad = 1) (csrc/dw_branches.hip)
def test_the_branch_sets_of_the_table_are_the_library_s():
    assert D.DWB_SETS == train_ops._DWB_SETS


@pytest.mark.parametrize("name", D.names("dwb", pred=lambda c: "unused" not in c))
def test_dw_branches_dgrad_sums_the_branches(name):
    c = D.BY_NAME[name]
    tdt, dt = _DT[c["dtype"]]
    inp = D.inputs(c)
    B, H, W, Cc, k0 = c["B"], c["H"], c["W"], c["C"], c["k0"]
    ks = D.DWB_SETS[k0]
    dzs = [_embed(dy, 8 * (j + 1), j % 2 == 0) for j, dy in enumerate(inp["dys"])]              # a different pixel stride per dz_j
    wps = [train_ops._packed_dw(_nonleaf(w), Cc, k, 1, dt, DEV) for w, k in zip(inp["ws"], ks)]
    out = _Out((B, H, W, Cc), tdt)
    P4, I4 = train_ops._PTR4, train_ops._INT4
    lib.check(lib.load().maf_dw_branches(P4(*[t.data_ptr() for t in dzs]), I4(*[t.stride(2) for t in dzs]), P4(out.slice_ptr), I4(out.stride),
                                         P4(*[t.data_ptr() for t in wps]), len(ks), k0, B, H, W, Cc, dt, 1, _stream()))
    torch.cuda.synchronize()
    _check(c, out.got(), name, "maf_dw_branches (dgrad)", out)


@pytest.mark.parametrize("name", D.names("dwb", pred=lambda c: "unused" in c))
def test_dw_branches_backward_with_an_unused_branch(name):
    """train_ops.dw_branches(...).backward with one branch's output out of the graph: dX is the sum over the others.  autograd MATERIALISES the missing gradient (the
    Function does not call ctx.set_materialize_grads(False)), so backward gets a zero tensor, not None: the `dy is None` branch of _DWBranches.backward, which would
    allocate the zeros itself (train_ops._tzeros), is unreachable from autograd and is asserted NOT to have run — what is checked is the zero dz on its way through
    T.nhwc and the merged launch."""
    c = D.BY_NAME[name]
    inp = D.inputs(c)
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    x0 = int_case((B, H, W, Cc), torch.Generator().manual_seed(c["seed"]), n_terms=81)
    n0 = train_ops.stats.get("native_dw_branches", 0)
    own_zeros, tz = [], train_ops._tzeros

    def counting(*a, **k):
        if a and tuple(a[0]) == (B, Cc, H, W):
            own_zeros.append(a[0])
        return tz(*a, **k)

    with _no_plan():
        x = _nchw(x0.to(DEV)).requires_grad_(True)
        ws = [torch.nn.Parameter(w.to(DEV)) for w in inp["ws"]]
        outs = train_ops.dw_branches(x, ws)
        used = [j for j in range(len(ws)) if j != c["unused"]]
        train_ops._tzeros = counting
        try:
            torch.autograd.backward([outs[j] for j in used], [_nchw(_embed(inp["dys"][j], 8 * (j + 1), True)) for j in used])
            torch.cuda.synchronize()
        finally:
            train_ops._tzeros = tz
    assert train_ops.stats.get("native_dw_branches", 0) == n0 + 1, "the merged launch did not run"
    assert not own_zeros, "backward was handed None for the unused branch: autograd no longer materialises it, and this test now runs the other route"
    _check(c, x.grad.permute(0, 2, 3, 1), name, "_DWBranches.backward")
