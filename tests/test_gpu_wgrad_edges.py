"""-m gpu: the weight-gradient kernels at their dispatch edges, straight through the C ABI, EXACTLY (references: tests/wgrad_ref.py, checked by test_wgrad_ref_host.py).

maf_conv_wgrad (csrc/wgrad.hip: wgrad_tr_kernel in its twelve (TI, NJ) forms, channel chunks of inputs wider than 256 channels, the replica workspace and its fold,
the nine-taps kernel, the patch form), maf_grad_fold, maf_dw_wgrad (csrc/dw_wgrad_mfma.hip and the vector kernel of csrc/train_ops.hip) and maf_dw_wgrad31.

Every call works on channel slices of wider NHWC buffers whose other channels are NaN, with a NaN pixel before the first and after the last pixel of each tensor: a
read outside the slice poisons the result.  dW is NOT zero on entry (the entry points accumulate: train_conv._wgrad adds straight into a non-zero exchange bucket) and
lies between guard floats that must come back untouched.

Family E (exact): inputs are small integers (wgrad_ref.int_case), so every product and partial sum is an integer below 2^22 and the fp32 result must be
`pre + ref` bit for bit whatever the order of chunks, replicas and atomics; the reference is summed in float64 (exact below 2^53) and converted through int64.
Family B (bound): wgrad_ref.wide_case inputs, n_terms <= 4096, dW = 0 on entry, per element |got - ref| <= ulp32(ref) + 2 * n_terms * 2^-24 * S (op_ref.K_CONV's
two units: the fp32 accumulation in any order, and the MFMA's internal order).

The parametrize lists name, beside each shape, the branch of the dispatch it is there for (wgrad_launch / maf_conv_wgrad / maf_dw_wgrad): when a threshold moves,
that comment says which case to move with it.  No MAF_* override is set: the branches are reached by shape.

Largest err / bound seen per entry point (family B, MI355X; the bound is derived, these are only what it left unused):
    maf_conv_wgrad   0.076   (16 -> 48, k 3 s 2, 5 x 7 x 1, n_terms 20; the 1x1 tile forms: 0.0092 at 200 -> 72)
    maf_dw_wgrad     0.0018  (fp32 vector kernel, k 7; matrix-core kernel 0.0010, fp16 vector kernel 0.0001)
"""
import pytest
import torch

from maf_yolo_amd import lib

import op_ref
from wgrad_ref import conv_wgrad_ref, dw_wgrad_ref, int_case, wide_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
GUARD = 64                      # floats on either side of dW (keeps dW 256-byte aligned)
SENTINEL = -12345.0
_SIDE = []


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _side_stream():
    """ONE second stream for the whole module: the library keeps a workspace slot per (device, stream) for the life of the process."""
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _embed(t, pad, front):
    """t [..., C] -> the same values as a channel slice of a buffer with pixel stride C + pad; the other channels, and one pixel before and after, are NaN."""
    C = t.shape[-1]
    npix = t.numel() // C
    buf = torch.full((npix + 2, C + pad), float("nan"), dtype=t.dtype, device=t.device)
    o = pad if front else 0
    buf[1:-1, o:o + C] = t.reshape(npix, C)
    return buf[1:-1].view(*t.shape[:-1], C + pad)[..., o:o + C]


def _guarded(pre):
    """(buffer, view): `pre` copied between two runs of GUARD sentinel floats."""
    buf = torch.full((pre.numel() + 2 * GUARD,), SENTINEL, dtype=F32, device=pre.device)
    view = buf[GUARD:GUARD + pre.numel()].view(pre.shape)
    view.copy_(pre)
    return buf, view


def _pre(shape, g):
    return torch.randint(-4, 5, tuple(shape), generator=g, device=DEV).float()


def _assert_exact(buf, got, want, tag):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "%s: wrote outside dW" % tag
    if torch.equal(got, want):
        return
    d = got.double() - want.double()
    bad = ~(d == 0)
    idx = bad.nonzero()[:12].tolist()
    pytest.fail("%s: %d of %d elements differ (%d NaN); max |diff| %s; first (index, got - want): %s" % (
        tag, int(bad.sum()), bad.numel(), int(torch.isnan(d).sum()), float(d[~torch.isnan(d)].abs().max()) if bool((~torch.isnan(d)).any()) else None,
        [(i, float(d[tuple(i)])) for i in idx]))


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _stream_ptr(stream):
    return (stream or torch.cuda.current_stream()).cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------------- maf_conv_wgrad
def _conv_inputs(B, Hs, Ws, cin, cout, k, s, g, make, xpad=8, dpad=16):
    Ho, Wo = _out(Hs, k, s), _out(Ws, k, s)
    kw = {"n_terms": B * Ho * Wo} if make is int_case else {}
    x = _embed(make((B, Hs, Ws, cin), g, **kw), xpad, True)
    dy = _embed(make((B, Ho, Wo, cout), g, **kw), dpad, False)
    return x, dy, Ho, Wo


def _conv_launch(x, dy, k, s, dw, stream=None):
    B, Hs, Ws, cin = x.shape
    _, Ho, Wo, cout = dy.shape
    lib.check(lib.load().maf_conv_wgrad(x.data_ptr(), x.stride(2), dy.data_ptr(), dy.stride(2), B, Ho, Wo, Hs, Ws, cin, cout, k, s, lib.F16, dw.data_ptr(), _stream_ptr(stream)))


def _conv_exact(B, Hs, Ws, cin, cout, k, s, seed=0, xpad=8, dpad=16):
    g = _gen(1000 * cin + cout + 7 * Hs + Ws + seed)
    x, dy, Ho, Wo = _conv_inputs(B, Hs, Ws, cin, cout, k, s, g, int_case, xpad, dpad)
    ref, _ = conv_wgrad_ref(x, dy, k, s, exact=True)
    pre = _pre(ref.shape, g)
    buf, dw = _guarded(pre)
    _conv_launch(x, dy, k, s, dw)
    torch.cuda.synchronize()
    _assert_exact(buf, dw, pre + ref.float(), "conv_wgrad %d -> %d k %d s %d on %d x %d x %d" % (cin, cout, k, s, B, Hs, Ws))


def _check_bound(got, ref, S, n_terms, entry, tag):
    assert n_terms <= 4096
    bound = op_ref.ulp(ref, f32=True) + op_ref.K_CONV * n_terms * 2.0 ** -24 * S
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    print("wgrad-B %s %s: n_terms %d, max err / bound %.4f" % (entry, tag, n_terms, ratio))
    assert bool((err <= bound).all()), "%s %s: err / bound %.4f" % (entry, tag, ratio)


def _conv_bound(B, Hs, Ws, cin, cout, k, s):
    g = _gen(1000 * cin + cout + 7 * Hs + Ws + 1)
    x, dy, Ho, Wo = _conv_inputs(B, Hs, Ws, cin, cout, k, s, g, wide_case)
    ref, S = conv_wgrad_ref(x, dy, k, s)
    buf, dw = _guarded(torch.zeros(ref.shape, device=DEV))
    _conv_launch(x, dy, k, s, dw)
    torch.cuda.synchronize()
    _check_bound(dw, ref, S, B * Ho * Wo, "maf_conv_wgrad", "%d -> %d k %d s %d on %d x %d x %d" % (cin, cout, k, s, B, Hs, Ws))


# (a) k = 1, stride 1, M = 200 pixels (three full 64-pixel steps and one of 8): every MAF_WG(TI, NJ) line of wgrad_launch.
# tci = ceil(Cin / 16) -> WJ = 1 / 2 / 4 for tci = 1 / 2..3 / >= 4, NJ = ceil(tci / WJ), WI = 4 / WJ; want = ceil(ceil(Cout / 16) / WI) -> TI = 1, 2, 4 (want >= 3)
TR_FORMS = [(16, 16),     # WJ 1 WI 4: TI = 1, NJ = 1
            (16, 80),     # 5 co tiles / 4 -> TI = 2, NJ = 1
            (16, 144),    # 9 co tiles / 4 -> TI = 4, NJ = 1
            (40, 24),     # tci 3 -> WJ 2, NJ = 2; WI 2: TI = 1 (the third ci tile holds 8 channels, the fourth none)
            (40, 56),     # TI = 2, NJ = 2
            (40, 88),     # 6 co tiles / 2 -> TI = 4, NJ = 2
            (136, 8),     # tci 9 -> WJ 4, NJ = 3; WI 1: TI = 1
            (136, 24),    # TI = 2, NJ = 3
            (136, 40),    # TI = 4 (3 co tiles, the fourth empty), NJ = 3
            (200, 16),    # tci 13 -> NJ = 4; TI = 1; the last 16-channel ci tile holds 8 channels
            (200, 32),    # TI = 2, NJ = 4
            (200, 72)]    # 5 co tiles -> TI = 4, gy = 2 (the second block row holds one tile of 8 channels), NJ = 4


@pytest.mark.parametrize("cin,cout", TR_FORMS)
def test_conv1x1_wgrad_every_tile_form_is_exact(cin, cout):
    _conv_exact(2, 10, 10, cin, cout, 1, 1)


@pytest.mark.parametrize("cin,cout", [(16, 80), (40, 88), (200, 72)])       # (TI, NJ) = (2, 1), (4, 2), (4, 4)
def test_conv1x1_wgrad_tile_forms_within_the_fp32_bound(cin, cout):
    _conv_bound(2, 10, 10, cin, cout, 1, 1)


# (b) channel chunks of inputs wider than 256 channels (maf_conv_wgrad: nchunk = ceil(Cin / 256), cchunk = ceil(Cin / nchunk) to whole 16-channel tiles) and pixel chunks
CHUNKS = [(1, 10, 13, 264, 40, 1, 1),      # chunks 144 + 120, M = 130: two full steps and one of 2 pixels
          (1, 10, 13, 520, 24, 1, 1),      # chunks 176 + 176 + 168 (the last ci tile of the last chunk holds 8 channels)
          (2, 9, 7, 264, 40, 3, 2),        # the same chunks under nine gathered taps: blockIdx.z = chunk * 9 + tap
          (2, 9, 7, 520, 24, 3, 2),
          (2, 51, 49, 520, 136, 3, 2)]     # M = 2 * 26 * 25 = 1300 (21 steps), gy = 3, gz = 27: fill = 1024 / 81 = 12 < 21 -> 128-pixel chunks, the last one of 20 pixels


@pytest.mark.parametrize("B,Hs,Ws,cin,cout,k,s", CHUNKS)
def test_conv_wgrad_channel_and_pixel_chunks_are_exact(B, Hs, Ws, cin, cout, k, s):
    _conv_exact(B, Hs, Ws, cin, cout, k, s)


# (c) the replica workspace of wgrad_tr_kernel and its fold: gx >= 256 pixel chunks and R = 8 copies (a small dW).  gx = min(sqrt(steps * 360000 / atomics), fill, steps),
# then chunk = ceil(steps / gx) steps and gx = ceil(M / chunk)
REPLICAS = [(1, 1, 16421, 8, 8, 1, 1),       # steps 257, atomics 256: gx = 257 one-step chunks -> copies
            (2, 259, 255, 24, 48, 1, 2),     # M = 2 * 130 * 128 = 33280, steps 520, atomics 1536: sqrt -> 349, two-step chunks, gx = 260 -> copies, gathered rows
            (2, 191, 190, 24, 48, 1, 2)]     # M = 18240, steps 285: sqrt -> 258, two-step chunks, gx = 143 < 256: the same layer just BELOW the copies' threshold


@pytest.mark.parametrize("B,Hs,Ws,cin,cout,k,s", REPLICAS)
def test_conv_wgrad_replica_fold_leaves_its_copies_zero_and_keeps_streams_apart(B, Hs, Ws, cin, cout, k, s):
    """Two launches back to back on the current stream (different inputs, no synchronisation between them), then one on a second stream: all three exact on a non-zero
    dW — the fold left the copies zero for the second launch, and the second stream got a slot of its own."""
    g = _gen(cin + Hs)
    runs = []
    for i in range(3):
        x, dy, Ho, Wo = _conv_inputs(B, Hs, Ws, cin, cout, k, s, g, int_case)
        ref, _ = conv_wgrad_ref(x, dy, k, s, exact=True)
        pre = _pre(ref.shape, g)
        runs.append((x, dy, pre, ref) + _guarded(pre))
    torch.cuda.synchronize()
    side = _side_stream()
    for i, (x, dy, pre, ref, buf, dw) in enumerate(runs):
        if i < 2:
            _conv_launch(x, dy, k, s, dw)
        else:
            with torch.cuda.stream(side):
                _conv_launch(x, dy, k, s, dw, side)
    torch.cuda.synchronize()
    for i, (x, dy, pre, ref, buf, dw) in enumerate(runs):
        _assert_exact(buf, dw, pre + ref.float(), "conv_wgrad %d -> %d s %d, M %d, launch %d%s" % (cin, cout, s, B * _out(Hs, k, s) * _out(Ws, k, s), i, " (second stream)" if i == 2 else ""))


# (d), (e) the small 3x3 stride-2 maps (M < 100000: no patch form)
SMALL_MAPS = [(3, 13, 11),      # 7 x 6: an ordinary small map, M = 126: one full step and one of 62 pixels
              (9, 5, 3),        # 3 x 2: fewer than 64 output pixels per image — the one staging step spans all nine images (`while (oy >= Ho)`)
              (5, 7, 1)]        # 4 x 1: Wo = 1, every output row is one pixel; taps kx = 0, 2 see only padding

# wgrad_launch takes wgrad_taps_kernel for ntaps = 9, one ci tile (Cin <= 16) and Cout <= 64 (its dY staging: 2 items per thread); tpw = ceil(9 * co tiles / 4)
NINE_TAPS = [(8, 24), (16, 24),       # 2 co tiles: tpw 5 -> launch_taps<5>
             (8, 48), (16, 48),       # 3 co tiles: tpw 7 -> launch_taps<8>
             (8, 64), (16, 64),       # 4 co tiles: tpw 9 -> launch_taps<16>; dY fills the 512 staging items exactly
             (8, 80), (16, 80),       # 5 co tiles: dY needs 640 items -> NOT the taps kernel: wgrad_tr_kernel<2, 1>, gz = 9 (before the fix of the rule: rows 51.. of dY unstaged)
             (8, 112), (16, 112)]     # 7 co tiles (896 items): the widest layer the old rule (9 * co tiles <= 64) let in -> wgrad_tr_kernel<2, 1>


@pytest.mark.parametrize("B,Hs,Ws", SMALL_MAPS)
@pytest.mark.parametrize("cin,cout", NINE_TAPS)
def test_conv3x3s2_wgrad_one_input_tile_is_exact(cin, cout, B, Hs, Ws):
    _conv_exact(B, Hs, Ws, cin, cout, 3, 2)


@pytest.mark.parametrize("B,Hs,Ws", SMALL_MAPS)
def test_conv3x3s2_wgrad_nine_taps_within_the_fp32_bound(B, Hs, Ws):
    _conv_bound(B, Hs, Ws, 16, 48, 3, 2)


# tap-per-workgroup form (wgrad_tr_kernel with gather, blockIdx.z = tap) on the same maps
TAP_PER_WG = [(96, 64, 3),      # tci 6 -> WJ 4, NJ 2; 4 co tiles -> TI 4
              (24, 48, 3),      # two ci tiles: too wide for the nine-taps kernel, too few pixels for the patch form
              (24, 48, 1)]      # k = 1 stride 2: tap0 = 4, the centre tap of the pad-1 geometry reads (2 oy, 2 ox)


@pytest.mark.parametrize("B,Hs,Ws", SMALL_MAPS)
@pytest.mark.parametrize("cin,cout,k", TAP_PER_WG)
def test_conv_wgrad_tap_per_workgroup_on_tiny_maps_is_exact(cin, cout, k, B, Hs, Ws):
    _conv_exact(B, Hs, Ws, cin, cout, k, 2)


# (f) patch form (maf_conv_wgrad: k = 3, Cin <= 48, Cout <= 64, M >= 100000); always through the eight copies and the fold
PATCH = [(2, 451, 500, 8, 24, 0, 8),       # ntj 1, nti 2: launch_patch<3, 2, 4, 3, 2, 4, 4>, odd Hs: the last tile row is ragged
         (2, 452, 450, 24, 48, 8, 0),      # ntj 2, nti 3: launch_patch<3, 3, 2, 2, 1, 2, 8>
         (2, 450, 455, 48, 64, 0, 0),      # ntj 3, nti 4: launch_patch<4, 4, 2, 4, 1, 2, 8>
         (3, 372, 370, 48, 48, 16, 16),    # ntj 3, nti 3: the last form with one co tile unused
         (1, 701, 603, 24, 48, 8, 16)]     # B = 1, odd sizes: 351 x 302, tilesX = 19 with a last tile of 14 columns


@pytest.mark.parametrize("B,Hs,Ws,cin,cout,xpad,dpad", PATCH)
def test_conv3x3s2_wgrad_patch_form_is_exact(B, Hs, Ws, cin, cout, xpad, dpad):
    _conv_exact(B, Hs, Ws, cin, cout, 3, 2, xpad=max(xpad, 8), dpad=max(dpad, 8))


# ----------------------------------------------------------------------------------------------------------------------------------------- maf_grad_fold
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("co_p,ci_p,cout,cin", [(72, 8, 68, 3),       # both channel counts padded: rows and columns of src to skip
                                                (48, 24, 48, 24)])     # nothing padded: a plain transpose
@pytest.mark.parametrize("taps", [1, 9])
def test_grad_fold_moves_the_valid_part_tap_last(taps, co_p, ci_p, cout, cin, accumulate):
    g = _gen(taps + co_p)
    src = torch.randn(taps, co_p, ci_p, generator=g, device=DEV)
    want_src = src[:, :cout, :cin].clone()
    src[:, cout:, :] = float("nan")
    src[:, :, cin:] = float("nan")
    pre = torch.randn(cout, cin, taps, generator=g, device=DEV)
    buf, dst = _guarded(pre)
    lib.check(lib.load().maf_grad_fold(src.data_ptr(), taps, co_p, ci_p, dst.data_ptr(), cout, cin, accumulate, _stream_ptr(None)))
    torch.cuda.synchronize()
    want = want_src.permute(1, 2, 0)
    _assert_exact(buf, dst, pre + want if accumulate else want.contiguous(), "grad_fold taps %d (%d, %d) -> (%d, %d) accumulate %d" % (taps, co_p, ci_p, cout, cin, accumulate))


# ------------------------------------------------------------------------------------------------------------------------------------------ maf_dw_wgrad
def _dw_inputs(B, H, W, C, dtype, g, make, n=2, pad=8):
    kw = {"n_terms": B * H * W} if make is int_case else {}
    return [_embed(make((B, H, W, C), g, **kw).to(dtype), pad, i % 2 == 0) for i in range(n)]


def _dw_launch(x, dy, k, dw, reps):
    B, H, W, C = x.shape
    lib.check(lib.load().maf_dw_wgrad(x.data_ptr(), x.stride(2), dy.data_ptr(), dy.stride(2), B, H, W, C, k, lib.F16 if x.dtype == F16 else lib.F32, dw.data_ptr(), reps,
                                      _stream_ptr(None)))


# matrix-core kernel (csrc/dw_wgrad_mfma.hip): fp16, k in {3, 5, 7, 9}, W <= 96 = 32 SEGS; maf_dw_wgrad takes it for k >= 5, or H W <= 400, or H W <= 1600 with C <= 192
DW_MFMA = [(2, 12, 5, 8, 3, 1),       # W = 5: SEGS 1, a width below one 8-column group
           (2, 9, 32, 8, 5, 3),       # W = 32: SEGS 1 filled exactly
           (1, 9, 33, 8, 7, 1),       # W = 33: SEGS 2 with one column in the second segment
           (2, 7, 64, 8, 3, 3),       # W = 64: SEGS 2 filled exactly (k = 3 here by H W = 448 <= 1600)
           (1, 6, 65, 8, 9, 1),       # W = 65: SEGS 3
           (1, 10, 95, 72, 5, 3),     # W = 95: SEGS 3, not a multiple of 8; 9 channel groups: not a whole 128-byte line
           (2, 33, 96, 8, 9, 1),      # W = 96: the widest map; H = 33 under k = 9: several row bands, the last one ragged
           (3, 2, 20, 72, 9, 3),      # H = 2 < k = 9: the map is smaller than the filter, most taps see only padding
           (2, 2, 5, 8, 9, 1),        # H and W both below the filter
           (2, 20, 20, 72, 7, 1),     # the 20 x 20 maps of the model, 9 channel groups
           (1, 5, 96, 72, 3, 3),      # k = 3 at the full width
           (4, 7, 5, 8, 5, 1),        # a tiny map over four images
           (1, 17, 40, 8, 7, 3),      # W = 40: SEGS 2, 8 columns in the second segment
           (2, 3, 64, 72, 9, 1)]      # H = 3 < k with two full segments

# where maf_dw_wgrad changes kernels (no assertion on which one ran: both must be exact)
DW_BOUNDARY = [(1, 11, 96, 16, 5, 1),     # W = 96: the last width of the matrix-core kernel
               (1, 11, 97, 16, 5, 1),     # W = 97: the vector kernel
               (2, 20, 20, 288, 3, 3),    # k = 3 with H W = 400: matrix cores at any C
               (1, 40, 40, 192, 3, 1),    # k = 3 with H W = 1600 and C = 192: the last C on the matrix cores
               (1, 40, 40, 200, 3, 3)]    # C = 200: the first shape of that map on the vector kernel

# vector kernel (csrc/train_ops.hip dw_wgrad_kernel): k = 1, W > 96, fp32
DW_VECTOR_F16 = [(2, 13, 21, 24, 1, 1),       # k = 1 (the 1 x 1 branch's per-channel scale), ragged 8 x 16 tiles
                 (1, 160, 160, 64, 9, 3),     # H W >= 160^2: gmax = 8 channel groups, 8 * 9 * 4 = 288 items -> a 320-thread workgroup, 72 KB of LDS
                 (3, 13, 100, 16, 5, 1),      # W = 100, H = 13: ragged tiles both ways (7 x 2 tiles of 16 x 8)
                 (2, 13, 100, 16, 3, 3)]
DW_VECTOR_F32 = [(2, 12, 20, 12, 3, 1),       # fp32: 4-channel groups, C = 12 -> 3 groups in one block
                 (2, 12, 20, 12, 7, 3),
                 (8, 20, 20, 576, 9, 1)]      # 72 channel blocks of 2 groups: the workgroup cap (1024 / 72 -> 15 per block) is below the 48 (image, tile) pairs: each walks several


def _dw_exact(B, H, W, C, k, reps, dtype):
    g = _gen(B * 1000 + H * 10 + W + k)
    x, dy = _dw_inputs(B, H, W, C, dtype, g, int_case)
    ref, _ = dw_wgrad_ref(x, dy, k, exact=True)
    pre = _pre((reps, C, k * k), g)
    buf, dw = _guarded(pre)
    _dw_launch(x, dy, k, dw, reps)
    torch.cuda.synchronize()
    _assert_exact(buf, dw.sum(0), pre.sum(0) + ref.float(), "dw_wgrad k %d on %d x %d x %d x %d %s, %d replicas" % (k, B, H, W, C, dtype, reps))


@pytest.mark.parametrize("B,H,W,C,k,reps", DW_MFMA + DW_BOUNDARY + DW_VECTOR_F16)
def test_dw_wgrad_fp16_is_exact(B, H, W, C, k, reps):
    _dw_exact(B, H, W, C, k, reps, F16)


@pytest.mark.parametrize("B,H,W,C,k,reps", DW_VECTOR_F32)
def test_dw_wgrad_fp32_is_exact(B, H, W, C, k, reps):
    _dw_exact(B, H, W, C, k, reps, F32)


@pytest.mark.parametrize("B,H,W,C,k,dtype", [(1, 10, 95, 72, 5, "f16"),      # matrix-core kernel
                                             (3, 13, 100, 16, 5, "f16"),     # vector kernel, fp16 (v_fma_mix_f32)
                                             (2, 12, 20, 12, 7, "f32")])     # vector kernel, fp32
def test_dw_wgrad_within_the_fp32_bound(B, H, W, C, k, dtype):
    dtype = {"f16": F16, "f32": F32}[dtype]
    g = _gen(B * 1000 + H * 10 + W + k + 1)
    x, dy = _dw_inputs(B, H, W, C, dtype, g, wide_case)
    ref, S = dw_wgrad_ref(x, dy, k)
    buf, dw = _guarded(torch.zeros(1, C, k * k, device=DEV))
    _dw_launch(x, dy, k, dw, 1)
    torch.cuda.synchronize()
    _check_bound(dw[0], ref, S, B * H * W, "maf_dw_wgrad", "k %d on %d x %d x %d x %d %s" % (k, B, H, W, C, dtype))


# ---------------------------------------------------------------------------------------------------------------------------------------- maf_dw_wgrad31
DW31 = [(3, 21, 100, 16, False, 1, "f16"),      # ragged tiles both ways, several images
        (3, 21, 100, 72, True, 4, "f16"),       # 9 channel groups -> blocks of 5 + 4 groups (gmax 8 only for C >= 160); three dY tiles
        (3, 21, 100, 16, True, 4, "f32"),
        (1, 7, 5, 16, True, 1, "f16"),          # a map smaller than one tile (TH = 7)
        (1, 7, 5, 72, False, 4, "f32"),         # fp32: 18 groups of 4 channels
        (1, 7, 5, 16, False, 4, "f16"),
        (2, 40, 36, 72, True, 1, "f16"),        # W = 36: the third tile column holds 4 columns
        (2, 40, 36, 16, False, 4, "f16"),
        (2, 40, 36, 72, True, 4, "f32"),
        (2, 40, 36, 16, True, 1, "f32")]


@pytest.mark.parametrize("B,H,W,C,two,reps,dtype", DW31)
def test_dw_wgrad31_is_exact(B, H, W, C, two, reps, dtype):
    dtype = {"f16": F16, "f32": F32}[dtype]
    g = _gen(B * 1000 + H * 10 + C + reps)
    x, dya, dyb, dy1 = _dw_inputs(B, H, W, C, dtype, g, int_case, n=4)
    ra, rb, r1 = dw_wgrad_ref(x, dya, 3, exact=True)[0], dw_wgrad_ref(x, dyb, 3, exact=True)[0], dw_wgrad_ref(x, dy1, 1, exact=True)[0].view(C)
    pa, pb, p1 = _pre((reps, C, 9), g), _pre((reps, C, 9), g), _pre((reps, C), g)
    (ba, dwa), (bb, dwb), (b1, dw1) = _guarded(pa), _guarded(pb), _guarded(p1)
    lib.check(lib.load().maf_dw_wgrad31(x.data_ptr(), x.stride(2), dya.data_ptr(), dya.stride(2), dyb.data_ptr() if two else None, dyb.stride(2) if two else 0,
                                        dy1.data_ptr(), dy1.stride(2), B, H, W, C, lib.F16 if dtype == F16 else lib.F32, dwa.data_ptr(), dwb.data_ptr() if two else None,
                                        dw1.data_ptr(), reps, _stream_ptr(None)))
    torch.cuda.synchronize()
    tag = "dw_wgrad31 %d x %d x %d x %d %s two %s, %d replicas: " % (B, H, W, C, dtype, two, reps)
    _assert_exact(ba, dwa.sum(0), pa.sum(0) + ra.float(), tag + "3x3 a")
    _assert_exact(b1, dw1.sum(0), p1.sum(0) + r1.float(), tag + "1x1")
    if two:
        _assert_exact(bb, dwb.sum(0), pb.sum(0) + rb.float(), tag + "3x3 b")
    else:
        _assert_exact(bb, dwb, pb, tag + "3x3 b (absent: untouched)")
