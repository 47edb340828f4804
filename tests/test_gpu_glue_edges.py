"""-m gpu: the structural kernels of the train graph straight through the C ABI, bit for bit — maf_maxpool_forward / _backward, maf_upsample2x_forward / _backward,
maf_detect_join / _backward, maf_nhwc_sum, maf_colsum — against the CPU references of tests/glue_ref.py (cases and the branch each is there for: glue_ref.POOL, UP,
JOIN, SUM, COL; checked by tests/test_glue_ref_host.py on the very tensors used here).  No MAF_* override is set and no case compares one kernel path with another.

Harness: every tensor a kernel reads is a channel slice of a wider buffer whose other channels, and the pixel before and after, are NaN (the max-pool too: its
maximum is an explicit compare that lets a NaN through, so a NaN neighbour read by mistake shows); slices sit at the front or the back in turn.  Every tensor a kernel
writes is a slice of NaN in a buffer that holds a sentinel elsewhere, which must come back bit-identical; the argmax bytes and colsum's fp32 `out` (non-zero on
entry) lie between guard words.  A refused call passes only if it returns non-zero and every output is bit-identical afterwards.  A device error ends the session.

Everything is torch.equal except the detect join's class probabilities (fp64 sigmoid of the stored logit: one fp16 ulp / two fp32 ulps) and their gradient
(d (1 - y) y from the stored y: ulp_T(ref) + 3 * 2^-24 |ref|).

What ran on the MI355X (accepted / refused launches per entry point; every one of them passed):
    maf_maxpool_forward 18 / 8, maf_maxpool_backward 36 / 8 (every case once on the reference's argmax and once on the forward's)
    maf_upsample2x_forward 5 / 4, maf_upsample2x_backward 5 / 4        maf_detect_join 7 / 4, maf_detect_join_backward 21 / 4 (both gradients, d_cls null, d_reg null)
    maf_nhwc_sum 16 / 5        maf_colsum 58 / 3 (C 1 .. 256: 256 down to 1 slab per workgroup; the 1024-workgroup cap at 65600 x 129)
    Refused, every output bit-identical: max-pool k 1, k 16, stride > k, 2 pad > k, a window larger than the padded map, misaligned C / strides; upsample misaligned C /
    strides, B 0; join 0 and 5 levels, nc or nreg not a multiple of 4; nhwc_sum n 0, n 5, misaligned C / strides; colsum C 257, a stride below C, M 0.
Largest err / bound of the toleranced checks: join cls fp16 0.4995 (of one ulp), fp32 0.84 (of two ulps); d logits fp16 0.4999, fp32 0.43.
Everything else held bit for bit — y, the argmax bytes, dx (0 written over the NaN of the pixels no window covers), the -inf / NaN windows, the copies, the pads — no
sentinel or guard was touched and no NaN neighbour was read: nothing had to be fixed.
Wall time of the file on the MI355X: 3.7 s (129 tests).
"""
import ctypes as C

import pytest
import torch

from maf_yolo_amd import lib

import glue_ref as R
from test_gpu_fwd_edges import NAN, SENT, _Out, _Src, _assert_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
_LDT = {F16: lib.F16, F32: lib.F32}
TALLY = {}                      # entry point -> [accepted, refused]
WORST = {}                      # entry point -> largest err / bound of the toleranced checks
_DONE = set()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(entry, *args):
    rc = getattr(lib.load(), entry)(*args)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                  # a fault of the device: nothing more is started on it
        pytest.exit("the device reported %s after %s: stopping" % (e, entry), returncode=3)
    if rc == -3:                                               # MAF_E_HIP: the runtime turned the launch down — not a refusal of the library
        pytest.fail("HIP error from %s: %s" % (entry, lib.load().maf_last_error().decode()))
    t = TALLY.setdefault(entry, [0, 0])
    t[0 if rc == 0 else 1] += 1
    return rc


def _ok(entry, *args):
    rc = _call(entry, *args)
    assert rc == 0, (entry, rc, lib.load().maf_last_error().decode())


def _es(dtype):
    return 2 if dtype == F16 else 4


def _src(t, pad, front):
    """t [B, H, W, C] (or [M, C]) as a poisoned slice; .data: its first element"""
    if t.dim() == 2:
        t = t.view(1, 1, *t.shape)
    s = _Src(t.contiguous(), pad, front)
    s.data = s.ptr + s.coff * t.element_size()
    return s


def _dst(bhw, Cc, dtype, pad, front, init=None):
    """an output slice of NaN (or `init`, what an accumulating kernel reads) in a buffer of sentinels"""
    coff = pad if front else 0
    o = _Out(bhw, dtype, [(coff, Cc)], Cc + pad)
    if init is not None:
        o.buf[1:-1, coff:coff + Cc] = init.reshape(-1, Cc).to(DEV)
    o.data = o.ptr + coff * _es(dtype)
    o.before = o.buf.clone()
    return o


def _unchanged(o, tag):
    it = torch.int16 if o.buf.dtype == F16 else torch.int32
    assert torch.equal(o.buf.view(it), o.before.view(it)), "%s: a refused call wrote to its output" % tag


class _Bytes:
    """n bytes between guard bytes"""
    G = 32

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * self.G,), 0xA5, dtype=torch.uint8, device=DEV)
        if init is not None:
            self.buf[self.G:self.G + n] = init.reshape(-1).to(DEV)
        self.ptr = self.buf[self.G:].data_ptr()
        self.before = self.buf.clone()

    def val(self):
        return self.buf[self.G:self.G + self.n]

    def assert_guards(self, tag):
        assert bool((self.buf[:self.G] == 0xA5).all()) and bool((self.buf[-self.G:] == 0xA5).all()), "%s: a guard byte was written" % tag

    def assert_untouched(self, tag):
        assert torch.equal(self.buf, self.before), "%s: written" % tag


class _F32:
    """n floats between guard floats"""
    G = 8

    def __init__(self, init):
        self.n = init.numel()
        self.buf = torch.full((self.n + 2 * self.G,), SENT, dtype=torch.float32, device=DEV)
        self.buf[self.G:self.G + self.n] = init.to(DEV)
        self.ptr = self.buf[self.G:].data_ptr()
        self.before = self.buf.clone()

    def val(self):
        return self.buf[self.G:self.G + self.n]

    def assert_guards(self, tag):
        assert torch.equal(self.buf[:self.G], self.before[:self.G]) and torch.equal(self.buf[-self.G:], self.before[-self.G:]), "%s: a guard float was written" % tag

    def assert_untouched(self, tag):
        assert torch.equal(self.buf, self.before), "%s: written" % tag


def _ptrs(vals, n=4):
    return (C.c_void_p * max(n, len(vals)))(*vals)


def _ints(vals, n=4):
    return (C.c_int32 * max(n, len(vals)))(*[int(v) for v in vals])


def _same_bits(got, want, tag):
    """torch.equal on the bit patterns of NaN-free-or-not tensors: NaN must sit where the reference has NaN, everything else equal"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaN in %d places, the reference in %d" % (tag, int(gn.sum()), int(wn.sum()))
    _assert_exact(torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want), tag)


# ------------------------------------------------------------------------------------------------------------------------------------------ max-pool
def _pool_call(c, x, y, idx, dy, dx, **over):
    a = dict(c, **{k: v for k, v in over.items() if k in ("k", "s", "p", "H", "W", "C")})
    dt = _LDT[c["dtype"]]
    rf = _call("maf_maxpool_forward", x.data, x.stride + over.get("bump_x", 0), a["B"], a["H"], a["W"], a["C"], a["k"], a["s"], a["p"], dt, y.data, y.stride + over.get("bump_y", 0), idx.ptr, _stream())
    rb = _call("maf_maxpool_backward", dy.data, dy.stride + over.get("bump_y", 0), idx.ptr, a["B"], a["H"], a["W"], a["C"], a["k"], a["s"], a["p"], dt, dx.data, dx.stride + over.get("bump_x", 0), _stream())
    return rf, rb


def _run_pool(name):
    if name in _DONE:
        return
    c, i = R.POOL_BY[name], R.pool_inputs(name)
    y_ref, idx_ref, dx_ref = R.pool_reference(name)
    B, H, W, Cc, dt = c["B"], c["H"], c["W"], c["C"], c["dtype"]
    n = R.NGRP[dt]
    Ho, Wo = y_ref.shape[1], y_ref.shape[2]
    flip = c["idx"] % 2 == 0
    x, dy = _src(i["x"], n, flip), _src(i["dy"], 2 * n, not flip)
    y, dx = _dst((B, Ho, Wo), Cc, dt, 2 * n, flip), _dst((B, H, W), Cc, dt, n, not flip)
    idx = _Bytes(B * Ho * Wo * Cc)
    # forward, then the backward on the REFERENCE's argmax (the backward is checked on its own) and once more on the forward's
    _ok("maf_maxpool_forward", x.data, x.stride, B, H, W, Cc, c["k"], c["s"], c["p"], _LDT[dt], y.data, y.stride, idx.ptr, _stream())
    y.assert_rest_untouched(name + " y"), idx.assert_guards(name + " idx")
    _same_bits(y.got(), y_ref.to(dt).to(DEV), name + " y")
    _assert_exact(idx.val().view(B, Ho, Wo, Cc), idx_ref.to(DEV), name + " idx")
    for which, ib in (("reference idx", _Bytes(B * Ho * Wo * Cc, idx_ref)), ("forward idx", idx)):
        dx = _dst((B, H, W), Cc, dt, n, not flip)
        ib.before = ib.buf.clone()
        _ok("maf_maxpool_backward", dy.data, dy.stride, ib.ptr, B, H, W, Cc, c["k"], c["s"], c["p"], _LDT[dt], dx.data, dx.stride, _stream())
        dx.assert_rest_untouched(name + " dx")
        _assert_exact(dx.got(), dx_ref.to(dt).to(DEV), "%s dx (%s)" % (name, which))        # (every NaN of the slice overwritten: pixels in no window hold 0)
        ib.assert_untouched(name + " idx is read-only")
    _DONE.add(name)


@pytest.mark.parametrize("name", list(R.POOL_BY))
def test_maxpool(name):
    _run_pool(name)


@pytest.mark.parametrize("tag,over", R.POOL_REFUSED, ids=[t for t, _ in R.POOL_REFUSED])
def test_maxpool_refusals(tag, over):
    if ("pool", tag) in _DONE:
        return
    c = dict(B=2, H=6, W=6, C=16, dtype=F16, k=3, s=1, p=1)
    x, dy = _src(torch.zeros(2, 6, 6, 16, dtype=F16), 8, True), _src(torch.zeros(2, 6, 6, 16, dtype=F16), 8, True)
    y, dx = _dst((2, 6, 6), 16, F16, 8, True), _dst((2, 6, 6), 16, F16, 8, True)
    idx = _Bytes(2 * 6 * 6 * 16)
    rf, rb = _pool_call(c, x, y, idx, dy, dx, **over)
    assert rf == -1 and rb == -1, (tag, rf, rb)
    _unchanged(y, tag), _unchanged(dx, tag), idx.assert_untouched(tag)
    _DONE.add(("pool", tag))


# ------------------------------------------------------------------------------------------------------------------------------------------ upsample 2x
def _run_up(name):
    if name in _DONE:
        return
    c, i = R.UP_BY[name], R.up_inputs(name)
    B, H, W, Cc, dt = c["B"], c["H"], c["W"], c["C"], c["dtype"]
    n = R.NGRP[dt]
    y_ref, dx_ref = R.up_ref(i["x"], i["dy"])
    flip = c["idx"] % 2 == 0
    x, y = _src(i["x"], 2 * n, flip), _dst((B, 2 * H, 2 * W), Cc, dt, n, not flip)               # a slice source into a slot of a concat buffer
    _ok("maf_upsample2x_forward", x.data, x.stride, B, H, W, Cc, _LDT[dt], y.data, y.stride, _stream())
    y.assert_rest_untouched(name + " y")
    _assert_exact(y.got(), y_ref.to(DEV), name + " y")
    dy, dx = _src(i["dy"], n, not flip), _dst((B, H, W), Cc, dt, 2 * n, flip)
    _ok("maf_upsample2x_backward", dy.data, dy.stride, B, H, W, Cc, _LDT[dt], dx.data, dx.stride, _stream())
    dx.assert_rest_untouched(name + " dx")
    _assert_exact(dx.got(), dx_ref.to(dt).to(DEV), name + " dx")
    _DONE.add(name)


@pytest.mark.parametrize("name", list(R.UP_BY))
def test_upsample2x(name):
    _run_up(name)


@pytest.mark.parametrize("tag,over", R.UP_REFUSED, ids=[t for t, _ in R.UP_REFUSED])
def test_upsample2x_refusals(tag, over):
    if ("up", tag) in _DONE:
        return
    x, dy = _src(torch.zeros(1, 2, 2, 16, dtype=F16), 8, True), _src(torch.zeros(1, 4, 4, 16, dtype=F16), 8, True)
    y, dx = _dst((1, 4, 4), 16, F16, 8, True), _dst((1, 2, 2), 16, F16, 8, True)
    B, Cc = over.get("B", 1), over.get("C", 16)
    rf = _call("maf_upsample2x_forward", x.data, x.stride + over.get("bump_x", 0), B, 2, 2, Cc, lib.F16, y.data, y.stride + over.get("bump_y", 0), _stream())
    rb = _call("maf_upsample2x_backward", dy.data, dy.stride + over.get("bump_y", 0), B, 2, 2, Cc, lib.F16, dx.data, dx.stride + over.get("bump_x", 0), _stream())
    assert rf == -1 and rb == -1, (tag, rf, rb)
    _unchanged(y, tag), _unchanged(dx, tag)
    _DONE.add(("up", tag))


# ------------------------------------------------------------------------------------------------------------------------------------------ detect join
def _held(entry, got, ref, bound, tag):
    err = (got.double().cpu() - ref).abs()
    r = float((err / bound).max())
    r = r if r == r else float("inf")
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    print("GLUE %s | err / bound %.4f" % (tag, r))
    assert bool((err <= bound).all()), "%s: err / bound %.4f (%d NaN)" % (tag, r, int(torch.isnan(err).sum()))


def _run_join(name):
    if name in _DONE:
        return
    c, i, ref = R.JOIN_BY[name], R.join_inputs(name), R.join_reference(name)
    B, nc, nreg, dt, lv = c["B"], c["nc"], c["nreg"], c["dtype"], c["levels"]
    nl, A = len(lv), sum(lv)
    flip = c["idx"] % 2 == 0
    cls = [_src(t.view(B, 1, hw, nc), 4 * (1 + l % 2), flip ^ (l % 2 == 1)) for l, (t, hw) in enumerate(zip(i["cls"], lv))]      # strides: multiples of 4, not of 8
    reg = [_src(t.view(B, 1, hw, nreg), 4 * (2 - l % 2), flip ^ (l % 2 == 0)) for l, (t, hw) in enumerate(zip(i["reg"], lv))]
    co, ro = _dst((B, 1, A), nc, dt, 0, True), _dst((B, 1, A), nreg, dt, 0, True)
    _ok("maf_detect_join", _ptrs([s.data for s in cls]), _ints([s.stride for s in cls]), _ptrs([s.data for s in reg]), _ints([s.stride for s in reg]), _ints(lv), nl, B, nc, nreg,
        _LDT[dt], co.data, ro.data, _stream())
    co.assert_rest_untouched(name + " cls"), ro.assert_rest_untouched(name + " reg")
    _assert_exact(ro.got().reshape(B, A, nreg), ref["reg"].to(DEV), name + " reg")
    _held("maf_detect_join cls %s" % R.DTN[dt], co.got().reshape(B, A, nc), ref["cls"], ref["cls_bound"], name + " cls")
    # backward: the gradient maps padded to the 16-byte group, strides above the pad; then d_cls null, then d_reg null
    ncp, nrp = R.pad_to(nc, dt), R.pad_to(nreg, dt)
    y, dc, dr = _src(i["y"].view(B, 1, A, nc), 0, True), _src(i["d_cls"].view(B, 1, A, nc), 0, True), _src(i["d_reg"].view(B, 1, A, nreg), 0, True)
    for which in ("both", "d_cls null", "d_reg null"):
        gc = [_dst((B, 1, hw), ncp, dt, 4 * (1 + l % 2), flip ^ (l % 2 == 0)) for l, hw in enumerate(lv)]
        gr = [_dst((B, 1, hw), nrp, dt, 4 * (2 - l % 2), flip ^ (l % 2 == 1)) for l, hw in enumerate(lv)]
        _ok("maf_detect_join_backward", None if which == "d_cls null" else dc.data, None if which == "d_reg null" else dr.data, y.data, _ints(lv), nl, B, nc, nreg, _LDT[dt],
            _ptrs([o.data for o in gc]), _ints([o.stride for o in gc]), _ptrs([o.data for o in gr]), _ints([o.stride for o in gr]), ncp, nrp, _stream())
        tag = "%s backward (%s)" % (name, which)
        dl, dlb, dreg = R.split_levels(ref["dl"], lv), R.split_levels(ref["dl_bound"], lv), R.split_levels(ref["dreg"], lv)
        for l, hw in enumerate(lv):
            gc[l].assert_rest_untouched(tag + " d logits"), gr[l].assert_rest_untouched(tag + " d reg")      # channels beyond the pad keep the sentinel
            gotc, gotr = gc[l].got().reshape(B, hw, ncp), gr[l].got().reshape(B, hw, nrp)
            assert not bool(gotc[..., nc:].ne(0).any()) and not bool(gotr[..., nreg:].ne(0).any()), tag + ": a pad channel is not 0"
            if which == "d_cls null":
                assert not bool(gotc.ne(0).any()), tag + ": d logits not 0"
            else:
                _held("maf_detect_join_backward d logits %s" % R.DTN[dt], gotc[..., :nc], dl[l], dlb[l], "%s level %d" % (tag, l))
            if which == "d_reg null":
                assert not bool(gotr.ne(0).any()), tag + ": d reg not 0"
            else:
                _assert_exact(gotr[..., :nreg], dreg[l].to(DEV), "%s level %d d reg" % (tag, l))
    _DONE.add(name)


@pytest.mark.parametrize("name", list(R.JOIN_BY))
def test_detect_join(name):
    _run_join(name)


@pytest.mark.parametrize("tag,over", R.JOIN_REFUSED, ids=[t for t, _ in R.JOIN_REFUSED])
def test_detect_join_refusals(tag, over):
    if ("join", tag) in _DONE:
        return
    lv, nc, nreg, B = over.get("levels", (2, 1)), over.get("nc", 8), over.get("nreg", 8), 2
    na = max(len(lv), 1)
    A = max(sum(lv), 1)
    cls = [_src(torch.zeros(B, 1, 2, 8, dtype=F16), 8, True) for _ in range(na)]
    co, ro = _dst((B, 1, A), 8, F16, 0, True), _dst((B, 1, A), 8, F16, 0, True)
    rf = _call("maf_detect_join", _ptrs([s.data for s in cls], 5), _ints([s.stride for s in cls], 5), _ptrs([s.data for s in cls], 5), _ints([s.stride for s in cls], 5), _ints(lv, 5), len(lv), B,
               nc, nreg, lib.F16, co.data, ro.data, _stream())
    y = _src(torch.zeros(B, 1, A, 8, dtype=F16), 0, True)
    gc = [_dst((B, 1, 2), 8, F16, 8, True) for _ in range(na)]
    rb = _call("maf_detect_join_backward", y.data, y.data, y.data, _ints(lv, 5), len(lv), B, nc, nreg, lib.F16, _ptrs([o.data for o in gc], 5), _ints([o.stride for o in gc], 5),
               _ptrs([o.data for o in gc], 5), _ints([o.stride for o in gc], 5), 8, 8, _stream())
    assert rf == -1 and rb == -1, (tag, rf, rb)
    _unchanged(co, tag), _unchanged(ro, tag)
    for o in gc:
        _unchanged(o, tag)
    _DONE.add(("join", tag))


# ------------------------------------------------------------------------------------------------------------------------------------------ nhwc_sum
def _run_sum(name):
    if name in _DONE:
        return
    c, i = R.SUM_BY[name], R.sum_inputs(name)
    n, acc, dt, M, Cc = c["n"], c["acc"], c["dtype"], c["M"], c["C"]
    g = R.NGRP[dt]
    src = [_src(t, g * (1 + k % 3), (c["idx"] + k) % 2 == 0) for k, t in enumerate(i["src"])]                    # mixed strides per source
    dst = _dst((1, 1, M), Cc, dt, 2 * g, c["idx"] % 2 == 1, init=i["dst"] if acc else None)
    _ok("maf_nhwc_sum", _ptrs([s.data for s in src]), _ints([s.stride for s in src]), n, dst.data, dst.stride, M, Cc, _LDT[dt], acc, _stream())
    dst.assert_rest_untouched(name)
    _assert_exact(dst.got().reshape(M, Cc), R.sum_ref(i["src"], i["dst"], acc).to(dt).to(DEV), name)
    _DONE.add(name)


@pytest.mark.parametrize("name", list(R.SUM_BY))
def test_nhwc_sum(name):
    _run_sum(name)


@pytest.mark.parametrize("tag,over", R.SUM_REFUSED, ids=[t for t, _ in R.SUM_REFUSED])
def test_nhwc_sum_refusals(tag, over):
    if ("sum", tag) in _DONE:
        return
    src = [_src(torch.zeros(5, 16, dtype=F16), 8, True) for _ in range(5)]
    dst = _dst((1, 1, 5), 16, F16, 8, True, init=torch.ones(5, 16))
    rc = _call("maf_nhwc_sum", _ptrs([s.data for s in src], 5), _ints([s.stride + over.get("bump_x", 0) for s in src], 5), over.get("n", 2), dst.data, dst.stride + over.get("bump_y", 0), 5,
               over.get("C", 16), lib.F16, 1, _stream())
    assert rc == -1, (tag, rc)
    _unchanged(dst, tag)
    _DONE.add(("sum", tag))


# ------------------------------------------------------------------------------------------------------------------------------------------ colsum
def _run_col(name):
    if name in _DONE:
        return
    c, i = R.COL_BY[name], R.col_inputs(name)
    x = _src(i["x"], 3 + c["idx"] % 4, c["idx"] % 2 == 0)                                                        # any stride >= C: no alignment is asked for
    out = _F32(i["pre"])
    _ok("maf_colsum", x.data, x.stride, c["M"], c["C"], _LDT[c["dtype"]], out.ptr, _stream())
    out.assert_guards(name)
    _assert_exact(out.val(), (i["pre"].double() + i["x"].double().sum(0)).float().to(DEV), name)                 # pre + ref: integers below 2^24, one exact add
    _DONE.add(name)


@pytest.mark.parametrize("name", list(R.COL_BY))
def test_colsum(name):
    _run_col(name)


@pytest.mark.parametrize("tag,over", R.COL_REFUSED, ids=[t for t, _ in R.COL_REFUSED])
def test_colsum_refusals(tag, over):
    if ("col", tag) in _DONE:
        return
    x = _src(torch.zeros(4, 264, dtype=F16), 8, True)
    out = _F32(torch.ones(264))
    rc = _call("maf_colsum", x.data, over.get("stride", x.stride), over.get("M", 4), over.get("C", 8), lib.F16, out.ptr, _stream())
    assert rc == -1, (tag, rc)
    out.assert_untouched(tag)
    _DONE.add(("col", tag))


# ------------------------------------------------------------------------------------------------------------------------------------------ the tally
def test_every_case_ran_and_the_tally_is_the_expected_one():
    """Runs whatever case has not run yet, then: accepted and refused launches per entry point are exactly what the case lists imply.  Prints the tally."""
    for run, names in ((_run_pool, R.POOL_BY), (_run_up, R.UP_BY), (_run_join, R.JOIN_BY), (_run_sum, R.SUM_BY), (_run_col, R.COL_BY)):
        for nme in names:
            run(nme)
    for fn, lst in ((test_maxpool_refusals, R.POOL_REFUSED), (test_upsample2x_refusals, R.UP_REFUSED), (test_detect_join_refusals, R.JOIN_REFUSED), (test_nhwc_sum_refusals, R.SUM_REFUSED),
                    (test_colsum_refusals, R.COL_REFUSED)):
        for tag, over in lst:
            fn(tag, over)
    for entry, (a, n) in sorted(TALLY.items()):
        print("TALLY %-28s accepted %4d  refused %3d" % (entry, a, n))
    for entry, r in sorted(WORST.items()):
        print("WORST %-44s %.4f" % (entry, r))
    want = {"maf_maxpool_forward": [len(R.POOL), len(R.POOL_REFUSED)], "maf_maxpool_backward": [2 * len(R.POOL), len(R.POOL_REFUSED)],
            "maf_upsample2x_forward": [len(R.UP), len(R.UP_REFUSED)], "maf_upsample2x_backward": [len(R.UP), len(R.UP_REFUSED)],
            "maf_detect_join": [len(R.JOIN), len(R.JOIN_REFUSED)], "maf_detect_join_backward": [3 * len(R.JOIN), len(R.JOIN_REFUSED)],
            "maf_nhwc_sum": [len(R.SUM), len(R.SUM_REFUSED)], "maf_colsum": [len(R.COL), len(R.COL_REFUSED)]}
    assert TALLY == want, (TALLY, want)
