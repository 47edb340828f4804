"""Plain restatement of the data gradients of the training convs — csrc/conv_mfma_dgrad.hip (3x3 stride 2), the 1x1 conv kernels on a transposed weight pack (1x1, and 1x1
stride 2 scattered onto the even pixels), csrc/dwconv.hip on a flipped filter, csrc/dw_branches.hip (dwb_dgrad_kernel) and the RepVGG pair joined by maf_add_sub2 — and
EVERY case tests/test_gpu_dgrad_edges.py runs, as data.  Device-agnostic torch, float64; checked on the CPU by tests/test_dgrad_ref_host.py.

The kernels GATHER: an input pixel collects the output pixels whose windows cover it (parity classes, flipped filters).  The references here SCATTER — the literal
transpose of the forward conv, dx[b, s oy - k // 2 + ky, s ox - k // 2 + kx, ci] += dy[b, oy, ox, co] w[co, ci, ky, kx] wherever the target lies inside the image — so
they share no index arithmetic with the code under test.  Every function returns (dx, S, n_terms): S the same sum over absolute values, n_terms the largest number of
products summed into one element of dx.

As in tests/wgrad_ref.py, small-integer inputs (`int_case`) make every product and partial sum an integer far below 2^24: the fp32 accumulation is exact in any order,
and a result of magnitude <= 2048 is stored exactly in fp16, so the kernel must return THE integer (family E).  `wide_case` inputs are for the derived bound
|got - ref| <= ulp(ref) + K_CONV * n_terms * 2^-24 * S (family B).

The cases: `CASES`, a list of dicts (name, kind, family E / B, dtype, shape, seed, `why`: the branch of the dispatch the case exists for, `muts`: the mutations of
`MUTATIONS` that exist in it).  `inputs(case)` draws the tensors with a CPU generator (the GPU test copies them to the device: both files see the same numbers);
`reference(case, inp, ...)` is the case's data gradient, optionally with one mutation applied — what test_dgrad_ref_host.py uses to show that each case can tell a
wrong kernel from a right one."""
import functools

import torch

from wgrad_ref import _as_int, _tap_range, int_case, wide_case


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _finish(dx, S, cnt, per_tap, exact):
    return _as_int(dx, exact), _as_int(S, exact), int(cnt.max()) * per_tap


def _conv_scatter(dy, w, k, s, H, W, drop):
    """(dX, S, per-pixel count of the taps that land on it), float64."""
    assert (k, s) in ((1, 1), (1, 2), (3, 2))
    B, Ho, Wo, Cout = dy.shape
    assert tuple(w.shape[2:]) == (k, k) and w.shape[0] == Cout and Ho == _out(H, k, s) and Wo == _out(W, k, s)
    dd, wd = dy.double(), w.double()
    dx = torch.zeros(B, H, W, w.shape[1], dtype=torch.float64, device=dy.device)
    S = torch.zeros_like(dx)
    cnt = torch.zeros(H, W, dtype=torch.int64)
    for ky in range(k):
        y0, y1, iy = _tap_range(H, Ho, k, s, ky)
        for kx in range(k):
            x0, x1, ix = _tap_range(W, Wo, k, s, kx)
            if y1 <= y0 or x1 <= x0 or drop == (ky, kx):
                continue
            ys, xs = slice(iy, iy + s * (y1 - y0 - 1) + 1, s), slice(ix, ix + s * (x1 - x0 - 1) + 1, s)
            d = dd[:, y0:y1, x0:x1]
            dx[:, ys, xs] += torch.einsum("bhwo,oi->bhwi", d, wd[:, :, ky, kx])
            S[:, ys, xs] += torch.einsum("bhwo,oi->bhwi", d.abs(), wd[:, :, ky, kx].abs())
            cnt[ys, xs] += 1
    return dx, S, cnt


def conv_dgrad_ref(dy, w, k, s, H, W, exact=False, drop=None):
    """dy [B, Ho, Wo, Cout] NHWC, w [Cout, Cin, k, k] -> (dX [B, H, W, Cin] float64, S, n_terms) of the conv with kernel k, stride s, pad k // 2 over an H x W input,
    (k, s) in {(1, 1), (1, 2), (3, 2)}.  exact: int64 (integer inputs).  drop: a tap (ky, kx) left out (the host test's mutation)."""
    dx, S, cnt = _conv_scatter(dy, w, k, s, H, W, drop)
    return _finish(dx, S, cnt, dy.shape[-1], exact)


def dw_dgrad_ref(dy, w, k, exact=False, drop=None):
    """Depth-wise k x k, stride 1, pad k // 2: dy [B, H, W, C], w [C, 1, k, k] (or [C, k, k]) -> (dX, S, n_terms).  k = 1: a per-channel scale."""
    B, H, W, C = dy.shape
    dd, wd = dy.double(), w.double().reshape(C, k, k)
    dx = torch.zeros(B, H, W, C, dtype=torch.float64, device=dy.device)
    S = torch.zeros_like(dx)
    cnt = torch.zeros(H, W, dtype=torch.int64)
    for ky in range(k):
        y0, y1, iy = _tap_range(H, H, k, 1, ky)
        for kx in range(k):
            x0, x1, ix = _tap_range(W, W, k, 1, kx)
            if y1 <= y0 or x1 <= x0 or drop == (ky, kx):
                continue
            ys, xs = slice(iy, iy + y1 - y0), slice(ix, ix + x1 - x0)
            d = dd[:, y0:y1, x0:x1]
            dx[:, ys, xs] += d * wd[:, ky, kx]
            S[:, ys, xs] += d.abs() * wd[:, ky, kx].abs()
            cnt[ys, xs] += 1
    return _finish(dx, S, cnt, 1, exact)


def dw_branches_dgrad_ref(dys, ws, exact=False, drop=None):
    """sum_j dw_dgrad(dys[j], ws[j]) over the branches of a DilatedReparamBlock (kernel sizes ws[j].shape[-1]; the 1x1 branch is a per-channel scale).
    drop: (j, ky, kx)."""
    dx = S = None
    n = 0
    for j, (dy, w) in enumerate(zip(dys, ws)):
        a, s_, n_ = dw_dgrad_ref(dy, w, int(w.shape[-1]), exact, drop[1:] if drop is not None and drop[0] == j else None)
        dx, S, n = (a, s_, n_) if dx is None else (dx + a, S + s_, n + n_)
    return dx, S, n


def repvgg_dgrad_ref(dz3, dz1, w3, w1, H, W, exact=False, drop=None):
    """The data gradient of (conv3x3 s2 (x, w3), conv1x1 s2 (x, w1)) of one H x W input: (dX, S, n_terms, (dX3, S3, n3), (dX1, S1, n1)) — the sum and its two addends
    (the kernels round each addend to the storage type before maf_add_sub2 adds them).  drop: (0, ky, kx) a tap of w3, (1, 0, 0) the 1x1 branch."""
    d3, S3, c3 = _conv_scatter(dz3, w3, 3, 2, H, W, drop[1:] if drop is not None and drop[0] == 0 else None)
    d1, S1, c1 = _conv_scatter(dz1, w1, 1, 2, H, W, drop[1:] if drop is not None and drop[0] == 1 else None)
    a3, a1 = _finish(d3, S3, c3, dz3.shape[-1], exact), _finish(d1, S1, c1, dz1.shape[-1], exact)
    return a3[0] + a1[0], a3[1] + a1[1], int((c3 + c1).max()) * dz3.shape[-1], a3, a1


# --------------------------------------------------------------------------------------------------------------------------------------------- the cases
DWB_SETS = {3: (3, 3, 1), 5: (5, 3, 1), 7: (7, 5, 3), 9: (9, 7, 5, 3)}        # train_ops._DWB_SETS (checked by the GPU test)
MUTATIONS = ("tap", "noflip", "parity", "row", "col", "batch", "chunk")
CASES = []


def _muts(kind, kw):
    """The mutations that exist in a case: a depth-wise filter can be left unflipped, a stride-2 gradient has parities, a batch of one has no images to swap, a dY of
    fewer than 16 channels has no second 8-channel chunk, the one-pixel 3x3 map uses the centre tap alone (transposing the taps changes nothing)."""
    m = ["tap", "row", "col"]
    if kind in ("dw", "dwb"):
        m.append("noflip")
    if kind in ("conv1s2", "repvgg") or (kind == "conv3" and (kw["H"], kw["W"]) != (1, 1)):
        m.append("parity")
    if kw["B"] >= 2:
        m.append("batch")
    if kw.get("cout", kw.get("C", 0)) >= 16:
        m.append("chunk")
    return tuple(x for x in MUTATIONS if x in m)


def _case(kind, tag, why, family="E", dtype="f16", **kw):
    CASES.append(dict(kind=kind, name="%s-%s" % (kind, tag), why=why, family=family, dtype=dtype, seed=1000 + len(CASES), muts=_muts(kind, kw), **kw))


# 3x3 stride-2 data gradient (maf_launch_conv_mfma: the split parity-class form for even H and W, dg_mc = B H/2 W/2 pixels per class; else all nine taps per pixel)
for _B, _H, _W, _why in [(1, 2, 2, "dg_mc 1: one pixel per parity class"),
                         (3, 6, 14, "dg_mc 63: one short of a 64-pixel tile"),
                         (2, 8, 16, "dg_mc 64: one 64-pixel tile exactly"),
                         (1, 10, 26, "dg_mc 65: one pixel in the second tile"),
                         (1, 2, 254, "dg_mc 127: one short of a tile_p = 2 tile"),
                         (3, 2, 86, "dg_mc 129: one pixel past a tile_p = 2 tile"),
                         (2, 24, 48, "dg_mc 576: 9 tiles per class (36 in all): m_tile = (jj / nN) * 8 + xcd wraps, early return for m_tile >= nM")]:
    _case("conv3", "split-%dx%dx%d" % (_B, _H, _W), _why, B=_B, H=_H, W=_W, cin=24, cout=24)
for _H, _W in [(5, 8), (8, 5), (5, 7), (1, 1), (1, 6), (3, 2)]:
    _case("conv3", "unsplit-%dx%d" % (_H, _W), "odd H or W: every pixel walks all nine taps, ((sy | sx) & 1) picks them", B=2, H=_H, W=_W, cin=24, cout=24)
for _K in (8, 24, 48, 72, 200):
    _case("conv3", "K%d" % _K, "cout %d is no whole 32-channel k-step: the c0 < Cin ? c0 : 0 clamp against the packer's zero rows" % _K, B=2, H=4, W=6, cin=40, cout=_K)
for _K in (32, 128, 384):
    _case("conv3", "K%d" % _K, "cout %d: whole k-steps" % _K, B=2, H=4, W=6, cin=40, cout=_K)
_case("conv3", "K200-unsplit", "a ragged last k-step under all nine taps", B=2, H=5, W=7, cin=24, cout=200)
_case("conv3", "N8-image", "cin 8 with a 3-channel weight (the image): channels 3..7 of dX exactly 0", B=2, H=4, W=6, cin=8, cout=48, cin_w=3)
for _N in (24, 40, 200):
    _case("conv3", "N%d" % _N, "cin %d is no multiple of 16 tile_c: the ragged channel tile must not store past the slice" % _N, B=2, H=4, W=6, cin=_N, cout=48)
_case("conv3", "N128", "cin 128: whole channel tiles for every tile_c", B=2, H=4, W=6, cin=128, cout=48)
_case("conv3", "N200-unsplit", "the ragged channel tile under all nine taps", B=2, H=5, W=7, cin=200, cout=24)
_case("conv3", "f32", "mfma_f32_16x16x4f32: 4-channel chunks, 16-channel k-steps", dtype="f32", B=2, H=4, W=6, cin=24, cout=24)
_case("conv3", "f32-unsplit", "the fp32 instantiation under all nine taps", dtype="f32", B=2, H=5, W=7, cin=24, cout=24)
_case("conv3", "B-split", "the bound, split form, 4 taps x 384 channels", family="B", B=2, H=8, W=10, cin=40, cout=384)
_case("conv3", "B-unsplit", "the bound, all-taps form", family="B", B=2, H=5, W=7, cin=72, cout=200)
_case("conv3", "B-f32", "the bound in fp32", family="B", dtype="f32", B=2, H=4, W=6, cin=24, cout=72)

# 1x1 data gradient: the forward kernels on maf_pack_w1x1(transpose = 1), reduction dim kk = cout rounded up to 8, every candidate of train_ops.conv_candidates(M, kk, cin)
CONV1_SHAPES = [(68, 192), (81, 64), (1, 64), (3, 128), (80, 128), (576, 192), (192, 576), (24, 72)]            # (cout, cin); kk = 72, 88, 8, 8, 80, 576, 192, 24
_M_BHW = {15: (1, 3, 5), 16: (2, 2, 4), 17: (1, 1, 17), 63: (3, 3, 7), 65: (1, 5, 13), 4551: (3, 37, 41)}
for _co, _ci in CONV1_SHAPES:
    for _M in (15, 16, 17, 63, 65, 4551):
        _b, _h, _w = _M_BHW[_M]
        _case("conv1", "%dto%d-M%d" % (_co, _ci, _M), "M %d %s; K = %d%s" % (_M, {15: "one short of a 16-pixel tile", 16: "one 16-pixel tile", 17: "one pixel past it",
              63: "one short of a 64-pixel tile", 65: "one pixel past it", 4551: "72 tiles of 64 pixels, the last one of 7: the persistent forms loop; at cin 576 the tuner adds tile_p 2 / 4 generic and tile_p 2 LDS tiles"}[_M],
              -(-_co // 8) * 8, " (zero-filled by the packer from %d)" % _co if _co % 8 else ""), B=_b, H=_h, W=_w, cin=_ci, cout=_co)
_case("conv1", "f32", "the fp32 instantiation of the generic kernel on a transposed pack", dtype="f32", B=1, H=5, W=13, cin=64, cout=24)
_case("conv1", "B", "the bound: 576 terms", family="B", B=1, H=5, W=13, cin=192, cout=576)
_case("conv1", "B-68", "the bound with a zero-filled reduction tail", family="B", B=3, H=3, W=7, cin=192, cout=68)

# through autograd: _Conv1x1.backward with cout = 68 (the as_strided route of a registered zero-padded buffer against the F.pad route)
_case("conv1", "autograd-68", "_Conv1x1.backward: dY of 68 channels, read as 72 in place (train_ops.zero_padded) or padded by F.pad", B=2, H=5, W=7, cin=192, cout=68)

# 1x1 stride 2 alone and the RepVGG pair (train_ops.conv1x1s2 / repvgg_convs through autograd)
_case("conv1s2", "24to48", "the 1x1 gradient scattered onto the even pixels, odd pixels exactly 0", B=2, H=8, W=16, cin=24, cout=48)
_case("conv1s2", "8to24-image", "the image path: weight rows 3..7 absent, their gradient exactly 0", B=1, H=4, W=8, cin=8, cout=24, cin_w=3)
for _ci, _co, _cw, _why in [(24, 48, 24, "the generic pair: 3x3 gradient + maf_add_sub2 of the compact 1x1 gradient"),
                            (8, 24, 3, "the image: maf_stem_train forward, channels 3..7 of dX exactly 0"),
                            (96, 96, 96, "three k-steps per tap, tile_c 4 by the static rule")]:
    for _B, _H, _W in [(2, 8, 16), (1, 4, 8)]:
        _case("repvgg", "%dto%d-%dx%dx%d" % (_ci, _co, _B, _H, _W), _why, B=_B, H=_H, W=_W, cin=_ci, cout=_co, cin_w=_cw)
_case("repvgg", "B", "the bound of the pair: one more ulp of each addend (maf_add_sub2 rounds between them)", family="B", B=2, H=8, W=16, cin=24, cout=48, cin_w=24)

# depth-wise: csrc/dwconv.hip on maf_pack_dw(flip = 1).  Every k on every map (C walks 8, 24, 72, 200), then every C under every k on the 9 x 13 map
_DW_MAPS = [((2, 3), "a map smaller than the filter"), ((4, 4), "one 4-pixel strip per row"), ((9, 13), "W = 13: a last strip of one pixel"),
            ((20, 20), "the 20 x 20 map of the model"), ((33, 7), "H = 33: a ragged last tile row, W = 7: a strip of 3")]
_DW_C = [(8, "one channel group"), (24, "3 groups: a partial 128-byte line"), (72, "9 groups: choose_tile's channel block leaves a partial last block"),
         (200, "25 groups: 3 full 64-channel blocks and one of 8")]
_seen = set()
for _i, _k in enumerate((3, 5, 7, 9)):
    for _j, ((_H, _W), _why) in enumerate(_DW_MAPS):
        _C, _cw = _DW_C[(_i + _j) % 4]
        _seen.add((_k, _H, _W, _C))
        _case("dw", "k%d-%dx%d-C%d" % (_k, _H, _W, _C), "%s; C = %d: %s" % (_why, _C, _cw), B=2, H=_H, W=_W, C=_C, k=_k)
    for _C, _cw in _DW_C:
        if (_k, 9, 13, _C) not in _seen:
            _case("dw", "k%d-9x13-C%d" % (_k, _C), "C = %d: %s" % (_C, _cw), B=2, H=9, W=13, C=_C, k=_k)
_case("dw", "f32", "fp32: 4-channel groups", dtype="f32", B=2, H=9, W=13, C=12, k=5)
_case("dw", "B", "the bound: 81 terms", family="B", B=2, H=9, W=13, C=24, k=9)
_case("dw", "B-f32", "the bound in fp32", family="B", dtype="f32", B=2, H=4, W=4, C=12, k=7)

# depth-wise branches: maf_dw_branches(dgrad = 1), the sum over the branches kept in registers
for _i, _k0 in enumerate((3, 5, 7, 9)):
    for _j, ((_H, _W), _why) in enumerate([((6, 10), "H = 6 < the 16-row tile, W = 10: a last strip of two"), ((20, 24), "the measured 16 x 16 tile: ragged both ways"),
                                           ((3, 5), "a map smaller than the larger filters")]):
        _C = (24, 72, 200, 8)[(_i + _j) % 4]
        _case("dwb", "k%d-%dx%d-C%d" % (_k0, _H, _W, _C), "%s; C = %d" % (_why, _C), B=2, H=_H, W=_W, C=_C, k0=_k0)
_case("dwb", "f32", "fp32: 4-channel groups", dtype="f32", B=2, H=6, W=10, C=12, k0=5)
_case("dwb", "B", "the bound: 81 + 49 + 25 + 9 terms", family="B", B=2, H=6, W=10, C=24, k0=9)
for _k0 in (3, 9):
    _case("dwb", "autograd-k%d" % _k0, "_DWBranches.backward with one branch's output unused: autograd hands it a materialised zero dz (the Function does not turn that off, so its "
          "`dy is None` branch cannot be reached from autograd and is NOT run here), which goes through T.nhwc like any other", B=2, H=6, W=10, C=24, k0=_k0, unused=1)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(kind, family=None, pred=None):
    return [c["name"] for c in CASES if c["kind"] == kind and (family is None or c["family"] == family) and (pred is None or pred(c))]


def _draw(case, shape, g, n_terms, weight=False):
    if case["family"] == "E":
        t = int_case(shape, g, amp=3, n_terms=n_terms)
    else:
        t = wide_case(shape, g)
        if weight:
            t = (t.float() / 64).half()          # 2^-12 .. 1: sums of 4096 products of two wide operands would leave fp16's range
    return t.float() if weight or case["dtype"] == "f32" else t


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(c["seed"])
    kind, B, H, W = c["kind"], c["B"], c["H"], c["W"]
    if kind in ("dw", "dwb"):
        ks = (c["k"],) if kind == "dw" else DWB_SETS[c["k0"]]
        n = sum(k * k for k in ks)
        dys = [_draw(c, (B, H, W, c["C"]), g, n) for _ in ks]
        ws = [_draw(c, (c["C"], 1, k, k), g, n, True) for k in ks]
        if c.get("unused") is not None:
            dys[c["unused"]] = torch.zeros_like(dys[c["unused"]])
        return dict(dys=dys, ws=ws)
    cin, cout, cin_w = c["cin"], c["cout"], c.get("cin_w", c["cin"])
    if kind == "conv1":
        return dict(dys=[_draw(c, (B, H, W, cout), g, cout)], ws=[_draw(c, (cout, cin_w, 1, 1), g, cout, True)])
    Ho, Wo = H // 2 + H % 2, W // 2 + W % 2
    if kind == "conv3":
        return dict(dys=[_draw(c, (B, Ho, Wo, cout), g, 4 * cout)], ws=[_draw(c, (cout, cin_w, 3, 3), g, 4 * cout, True)])
    if kind == "conv1s2":
        return dict(dys=[_draw(c, (B, Ho, Wo, cout), g, cout)], ws=[_draw(c, (cout, cin_w, 1, 1), g, cout, True)])
    assert kind == "repvgg"
    return dict(dys=[_draw(c, (B, Ho, Wo, cout), g, 5 * cout) for _ in range(2)],
                ws=[_draw(c, (cout, cin_w, 3, 3), g, 5 * cout, True), _draw(c, (cout, cin_w, 1, 1), g, 5 * cout, True)])


def inputs(case):
    """{"dys": [dY per branch, NHWC, the case's dtype], "ws": [weights in the parameter's layout, fp32 holding fp16 values]} on the CPU.  Shared: do not write to them."""
    return _inputs(case["name"])


def _pad_ci(w, cin):
    """The weight as the kernels see it: absent input channels (the image's 3 of 8) are zero rows."""
    return w if w.shape[1] == cin else torch.cat([w, w.new_zeros(w.shape[0], cin - w.shape[1], *w.shape[2:])], 1)


def mutate_inputs(inp, what):
    """A copy of `inp` with dY damaged as a wrong kernel would read it: "row" / "col" the last row / column ignored, "batch" the images swapped, "chunk" the last whole
    8-channel chunk taken from chunk 0."""
    dys = [d.clone() for d in inp["dys"]]
    for d in dys:
        if what == "row":
            d[:, -1] = 0
        elif what == "col":
            d[:, :, -1] = 0
        elif what == "batch":
            d.copy_(d.flip(0))
        elif what == "chunk":
            c0 = (d.shape[-1] // 8 - 1) * 8
            assert c0 >= 8
            d[..., c0:c0 + 8] = d[..., :8]
        else:
            raise ValueError(what)
    return dict(dys=dys, ws=inp["ws"])


def reference(case, inp=None, exact=None, drop=None, noflip=False, parity=None):
    """(dX, S, n_terms, parts) of `case` on `inp` (default: its own inputs).  parts: ((dX3, S3, n3), (dX1, S1, n1)) for the RepVGG pair, else None.
    Mutations of the computation: drop = (branch, ky, kx) one tap left out; noflip: the depth-wise filters used as a correlation (unflipped) where the gradient is a
    convolution; parity = "taps": the 3x3 taps transposed (row parity taken for column parity), "sub2": the stride-2 1x1 gradient landed on the odd pixels."""
    inp = inputs(case) if inp is None else inp
    exact = case["family"] == "E" if exact is None else exact
    kind, H, W = case["kind"], case["H"], case["W"]
    dys, ws = inp["dys"], inp["ws"]
    if kind in ("dw", "dwb"):
        if noflip:
            ws = [w.flip(-1, -2) for w in ws]
        return dw_branches_dgrad_ref(dys, ws, exact, drop) + (None,)
    ws = [_pad_ci(w, case["cin"]) for w in ws]
    if parity == "taps":
        ws = [w.transpose(-1, -2) for w in ws]
    sub = drop[1:] if drop is not None else None
    if kind == "conv1":
        return conv_dgrad_ref(dys[0], ws[0], 1, 1, H, W, exact, sub) + (None,)
    if kind == "conv3":
        return conv_dgrad_ref(dys[0], ws[0], 3, 2, H, W, exact, sub) + (None,)
    if kind == "conv1s2":
        r = conv_dgrad_ref(dys[0], ws[0], 1, 2, H, W, exact, sub)
        return ((r[0].roll((1, 1), (1, 2)), r[1].roll((1, 1), (1, 2)), r[2]) if parity == "sub2" else r) + (None,)
    dx, S, n, a3, a1 = repvgg_dgrad_ref(dys[0], dys[1], ws[0], ws[1], H, W, exact, drop)
    if parity == "sub2":
        a1 = (a1[0].roll((1, 1), (1, 2)), a1[1].roll((1, 1), (1, 2)), a1[2])
        dx, S = a3[0] + a1[0], a3[1] + a1[1]
    return dx, S, n, (a3, a1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return reference(BY_NAME[name])


def case_reference(case):
    """reference(case) on its own inputs, computed once per process.  Shared: do not write to it."""
    return _reference(case["name"])
