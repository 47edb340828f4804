"""-m gpu: csrc/bn_sum.hip (the merged BatchNorm sum of a DilatedReparamBlock / RepVGGBlock, forward, STATS form and backward) straight through the C ABI, against the
fp64 reference of tests/bn_sum_ref.py — EXACTLY where the arithmetic allows it.  No case compares one kernel path with another.  Cases, families of inputs and the
branch each case is there for: bn_sum_ref.CASES (checked on the very tensors used here by tests/test_bn_sum_ref_host.py, which also recomputes the launcher's grid,
slice and replica arithmetic to show that every named branch is reached).  No MAF_* override is set: the branches are reached by shape.

Harness: every tensor a kernel reads (z_j, dy) is a channel slice of a wider buffer whose other channels, and the pixel before and after, are NaN; the slices sit at
the front or the back in turn and the pads (so the pixel strides) differ from tensor to tensor.  Every tensor a kernel writes (out, dz_j) is a slice of NaN in a buffer
that holds a sentinel elsewhere, which must come back bit-identical.  Every fp32 vector (gamma, beta, save_mean, save_rstd, running statistics, dgamma, dbeta, the
counter, both scratch buffers) lies between guard words; dgamma / dbeta start non-zero.  A refused call passes only if it returns the expected code and every output
and scratch buffer is bit-identical afterwards.  A device error ends the session (pytest.exit); nothing is retried.

Backward: every family-E case runs three calls on one scratch, phases p, 1 - p, p: each call gives the reference bit for bit (dgamma, dbeta = pre + ref for every M; dz
for M a power of two, within bn_ref.BARS otherwise), the half being left is all zero after every call (it held garbage before the first) and the half being used holds
nothing beyond the min(R, 16, 1024 / C) replicas the kernel may use.  Family B (one call): bn_ref.BARS, err_max per tensor.
Forward: three calls on every branch's own scratch, phases p, 1 - p, p — the first with the exact {sum z, sum z^2} written by the test over the replicas the kernel
reads, the other two with the sums maf_bn_stats accumulates into the half the call before cleared.  save_mean bit for bit, save_rstd and the running statistics within
one fp32 ulp, num_batches_tracked + 1, out within bn_ref.BARS (the `unit` family: bit for bit), the other half zero.  STATS form: the next BatchNorm's half gains
exactly the sums of the stored out (`unit`) or within BARS['stat'] of them.

What ran on the MI355X (157 cases: 144 = 9 group counts x 2 dtypes x 8 pixel counts, 4 of 257 groups, the 131072 x 64 one, 2 real-valued STATS cases, the largest C
of the six (nb, dtype); every one of them passed):
    maf_bn_sum_backward         487 accepted (3 x 155 family E + 22 family B), 13 refused
    maf_bn_sum_forward          360 accepted (3 x 120), 13 refused        maf_bn_sum_forward_stats   111 accepted (3 x 37), 13 refused
    maf_bn_stats                938 accepted (two per branch and case: the second and third forward call)
    Refused, nothing written, both scratch halves and every output bit-identical: nb 1, nb 5, C off the channel group (fp16, fp32), a misaligned stride, C 4104, phase 2
    (MAF_E_ARG) and C = 3416 / 2416 / 1864 (fp16), 3416 / 2412 / 1864 (fp32) for nb 2 / 3 / 4 (MAF_E_UNSUPPORTED), next to 3408 / 2408 / 1856 and 3412 / 2408 / 1860,
    which run and are checked for values in both directions.
Largest err / bar seen (family B and the toleranced forward checks; the bars are bn_ref.BARS, these are only what they left unused):
    backward dz fp16 0.018, fp32 0.0006; dgamma fp32 0.0008, dbeta fp32 0.0006 (fp16 storage: below 1e-4 of the bar)
    forward out fp16 0.055, fp32 0.038 (STATS form 0.015 / 0.0004); STATS sums of real-valued out: fp32 0.0005, fp16 below 1e-4 of the bar
Every family-E comparison held bit for bit, save_mean bit for bit, save_rstd and the running statistics within one ulp, no sentinel or guard was touched and no NaN
neighbour was read.  What had to be fixed was found by reading, before anything ran: check() took every C <= 4096 although the forward never raised its dynamic-LDS
limit and the backward raised it to 160 KiB only — a backward call past that failed at its apply launch after its statistics launch had added into the scratch
half.  check() now refuses (2 + 5 nb) C floats > 160 KiB with MAF_E_UNSUPPORTED before anything is launched, in both directions, and train_ops.bn_sum's gate
(train_bn.bn_sum_takes) sends those widths down the bn_act chain.
Wall time of the file on the MI355X: 7.5 s (349 tests).
"""
import ctypes as C

import pytest
import torch

from maf_yolo_amd import lib, train_bn

import bn_ref
import bn_sum_ref as R
from test_gpu_fwd_edges import SENT, _Out, _Src, _assert_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32
_LDT = {F16: lib.F16, F32: lib.F32}
_ACT = {None: lib.ACT_NONE, "relu": lib.ACT_RELU}
GARBAGE = 777.25
TALLY = {}                      # entry point -> [accepted, refused]
WORST = {}                      # entry point / tensor -> largest err / bar of the toleranced checks
_DONE = set()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(entry, *args):
    """the return code of an entry point, after the device has finished"""
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


def _rup(c):
    return -(-c // 256) * 256


class _Vec:
    """n words (fp32 by default) between guard words that hold the sentinel"""
    G = 8

    def __init__(self, init, dtype=torch.float32):
        init = init.to(dtype).reshape(-1)
        self.n = init.numel()
        self.buf = torch.full((self.n + 2 * self.G,), int(SENT) if dtype == torch.int64 else SENT, dtype=dtype, device=DEV)
        self.buf[self.G:self.G + self.n] = init.to(DEV)
        self.ptr = self.buf[self.G:].data_ptr()
        self.before = self.buf.clone()

    def val(self):
        return self.buf[self.G:self.G + self.n]

    def set(self, t):
        self.buf[self.G:self.G + self.n] = t.to(DEV)
        self.before = self.buf.clone()

    def assert_guards(self, tag):
        assert torch.equal(self.buf[:self.G], self.before[:self.G]) and torch.equal(self.buf[-self.G:], self.before[-self.G:]), "%s: a guard word was written" % tag

    def assert_untouched(self, tag):
        assert torch.equal(self.buf.view(torch.int32 if self.buf.dtype == torch.float32 else torch.int64), self.before.view(torch.int32 if self.buf.dtype == torch.float32 else torch.int64)), \
            "%s: written (%d words differ)" % (tag, int((self.buf != self.before).sum()))


def _ptrs(vals):
    return (C.c_void_p * max(4, len(vals)))(*vals)


def _ints(vals):
    return (C.c_int32 * max(4, len(vals)))(*[int(v) for v in vals])


def _src(t, dtype, j, flip):
    M, Cc = t.shape
    n = R.NGRP[dtype]
    s = _Src(t.view(1, 1, M, Cc), n * (1 + j % 2), bool((flip + j) % 2))
    s.data = s.ptr + s.coff * t.element_size()
    return s


def _out(M, Cc, dtype, j, flip):
    n = R.NGRP[dtype]
    pad = n * (1 + (j + 1) % 2)
    coff = pad if (flip + j) % 2 else 0
    o = _Out((1, 1, M), dtype, [(coff, Cc)], Cc + pad)
    o.data = o.ptr + coff * (2 if dtype == F16 else 4)
    return o


def _bar(entry, name, e, lim):
    r = e / lim
    r = r if r == r else float("inf")
    WORST[(entry, name)] = max(WORST.get((entry, name), 0.0), r)
    return r


def _within_ulp(got, ref, tag):
    """|got - ref| <= one fp32 ulp of the fp64 reference"""
    d = (got.double().cpu() - ref).abs()
    assert bool((d <= R.ulp32(ref)).all()), "%s: %.3f ulp" % (tag, float((d / R.ulp32(ref)).max()))


# ------------------------------------------------------------------------------------------------------------------------------------------ backward
class _Bwd:
    """the read-only side of a backward call: sources, per-branch vectors, the scratch [2][R][1 + nb][roundup(C, 256)]"""

    def __init__(self, nb, dtype, M, Cc, Rr, inp, flip, nalloc=None):
        na = nalloc or nb
        self.nb, self.dtype, self.M, self.C, self.R, self.flip, self.na = nb, dtype, M, Cc, Rr, flip, na
        self.z = [_src(inp["z"][j % len(inp["z"])], dtype, j, flip) for j in range(na)]
        self.dy = _src(inp["dy"], dtype, 1, flip + 1)
        self.vec = {k: [_Vec(inp[k][j % len(inp[k])]) for j in range(na)] for k in ("gamma", "beta", "mean", "rstd")}
        self.half = Rr * (1 + nb) * _rup(Cc)
        self.part = _Vec(torch.zeros(2 * self.half))
        self.pre = inp

    def outputs(self):
        dz = [_out(self.M, self.C, self.dtype, j, self.flip) for j in range(self.na)]
        dg = [_Vec(self.pre["pre_dgamma"][j % len(self.pre["pre_dgamma"])]) for j in range(self.na)]
        db = [_Vec(self.pre["pre_dbeta"][j % len(self.pre["pre_dbeta"])]) for j in range(self.na)]
        return dz, dg, db

    def call(self, outs, phase, acc, act, nb=None, Cc=None, dy_stride=None):
        dz, dg, db = outs
        v = self.vec
        return _call("maf_bn_sum_backward", self.dy.data, self.dy.stride if dy_stride is None else dy_stride, _ptrs([z.data for z in self.z]), _ints([z.stride for z in self.z]),
                     self.nb if nb is None else nb, self.M, self.C if Cc is None else Cc, _LDT[self.dtype], _ptrs([t.ptr for t in v["gamma"]]), _ptrs([t.ptr for t in v["beta"]]),
                     _ptrs([t.ptr for t in v["mean"]]), _ptrs([t.ptr for t in v["rstd"]]), _ptrs([o.data for o in dz]), _ints([o.stride for o in dz]),
                     _ptrs([t.ptr for t in dg]), _ptrs([t.ptr for t in db]), acc, self.part.ptr, self.R, phase, _ACT[act], _stream())

    def assert_read_only_intact(self, tag):
        for k, vs in self.vec.items():
            for t in vs:
                t.assert_untouched(tag + " " + k)


def _check_backward(c, fam, b, outs, ref, phase, tag):
    dz, dg, db = outs
    nb, M, Cc, dtype = c["nb"], c["M"], c["C"], c["dtype"]
    bar = bn_ref.BARS[dtype]["grad"]
    bad = []
    for j in range(nb):
        dz[j].assert_rest_untouched(tag + " dz%d" % j)
        dg[j].assert_guards(tag + " dgamma%d" % j), db[j].assert_guards(tag + " dbeta%d" % j)
        got_z = dz[j].got().reshape(M, Cc)
        pre_g, pre_b = b.pre["pre_dgamma"][j].to(DEV), b.pre["pre_dbeta"][j].to(DEV)
        if fam == "E":
            want_g = ref["dgamma"][j].float().to(DEV) + (pre_g if c["acc"] else 0)          # one fp32 add, as the kernel's
            want_b = ref["dbeta"][j].float().to(DEV) + (pre_b if c["acc"] else 0)
            _assert_exact(dg[j].val(), want_g, tag + " dgamma%d" % j)
            _assert_exact(db[j].val(), want_b, tag + " dbeta%d" % j)
            if R.is_pow2(M):
                _assert_exact(got_z, ref["dz_exact"][j].to(dtype).to(DEV), tag + " dz%d" % j)
                continue
            figs = [("dz", bn_ref.err_max(got_z, ref["dz"][j]))]
        else:
            figs = [("dz", bn_ref.err_max(got_z, ref["dz"][j])),
                    ("dgamma", bn_ref.err_max(dg[j].val().double().cpu() - (pre_g.double().cpu() if c["acc"] else 0), ref["dgamma"][j])),
                    ("dbeta", bn_ref.err_max(db[j].val().double().cpu() - (pre_b.double().cpu() if c["acc"] else 0), ref["dbeta"][j]))]
        assert bool(torch.isfinite(got_z).all()), tag + " dz%d: not finite" % j
        for name, e in figs:
            r = _bar("maf_bn_sum_backward", "%s %s" % (name, R.DTN[dtype]), e, bar)
            print("BNSUM %s | family %s %s%d %.3e (bar %.0e)" % (tag, fam, name, j, e, bar))
            if not r <= 1:
                bad.append((name, j, e, bar))
    assert not bad, (tag, bad)
    # the scratch: guards, the half being left all zero, nothing beyond the replicas the kernel may use in the half being used
    b.part.assert_guards(tag + " bpart")
    p = b.part.val()
    assert not bool(p[(1 - phase) * b.half:(2 - phase) * b.half].any()), tag + ": the half being left is not zero"
    used = R.replicas(Cc, c["R"]) * (1 + nb) * Cc
    assert not bool(p[phase * b.half + used:(phase + 1) * b.half].any()), tag + ": scratch beyond the replicas the kernel may use was written"
    if fam == "E":                                                                  # what the statistics launch left: the exact sums, over the replicas
        s = p[phase * b.half:phase * b.half + used].view(-1, 1 + nb, Cc).double().sum(0).cpu()
        assert torch.equal(s[0], ref["dbeta"][0]) and all(torch.equal(s[1 + j], ref["dgamma"][j]) for j in range(nb)), tag + ": the scratch half does not hold the exact sums"
    b.assert_read_only_intact(tag)


def _run_backward(name, fam):
    if (name, fam) in _DONE:
        return
    c = R.BY_NAME[name]
    inp, ref = R.backward_inputs(name, fam), R.backward_reference(name, fam)
    b = _Bwd(c["nb"], c["dtype"], c["M"], c["C"], c["R"], inp, c["idx"])
    p0 = c["idx"] % 2
    b.part.val()[(1 - p0) * b.half:(2 - p0) * b.half] = GARBAGE                  # the half the first call leaves
    for step, phase in enumerate((p0, 1 - p0, p0) if fam == "E" else (p0,)):
        outs = b.outputs()
        tag = "%s bwd %s call %d" % (name, fam, step)
        assert b.call(outs, phase, c["acc"], c["act"]) == 0, (tag, lib.load().maf_last_error().decode())
        _check_backward(c, fam, b, outs, ref, phase, tag)
    _DONE.add((name, fam))


@pytest.mark.parametrize("name", R.names(lambda c: "E" in c["bwd"]))
def test_backward_exact(name):
    _run_backward(name, "E")


@pytest.mark.parametrize("name", R.names(lambda c: "B" in c["bwd"]))
def test_backward_real_valued(name):
    _run_backward(name, "B")


# ------------------------------------------------------------------------------------------------------------------------------------------ forward
class _Fwd:
    def __init__(self, nb, dtype, M, Cc, Rr, inp, flip, nalloc=None, stats=False):
        na = nalloc or nb
        self.nb, self.dtype, self.M, self.C, self.R, self.flip, self.na = nb, dtype, M, Cc, Rr, flip, na
        self.z = [_src(inp["z"][j % len(inp["z"])], dtype, j, flip) for j in range(na)]
        self.vec = {k: [_Vec(inp[k][j % len(inp[k])]) for j in range(na)] for k in ("gamma", "beta")}
        self.inp = inp
        self.half = Rr * 2 * _rup(Cc)
        self.part = [_Vec(torch.zeros(2 * self.half)) for _ in range(na)]
        self.nhalf = Rr * 2 * _rup(Cc)
        self.next = _Vec(torch.zeros(2 * self.nhalf)) if stats else None

    def outputs(self):
        o = dict(out=_out(self.M, self.C, self.dtype, 1, self.flip))
        for k in ("mean", "rstd"):
            o[k] = [_Vec(torch.full((self.C,), GARBAGE)) for _ in range(self.na)]
        o["rm"] = [_Vec(self.inp["running_mean"][j % len(self.inp["running_mean"])]) for j in range(self.na)]
        o["rv"] = [_Vec(self.inp["running_var"][j % len(self.inp["running_var"])]) for j in range(self.na)]
        o["cnt"] = [_Vec(torch.tensor([41 + j]), torch.int64) for j in range(self.na)]
        return o

    def call(self, o, phases, act, eps, nphase=0, nb=None, Cc=None, out_stride=None):
        args = [_ptrs([z.data for z in self.z]), _ints([z.stride for z in self.z]), self.nb if nb is None else nb, self.M, self.C if Cc is None else Cc, _LDT[self.dtype],
                _ptrs([t.ptr for t in self.vec["gamma"]]), _ptrs([t.ptr for t in self.vec["beta"]]), float(eps), float(R.MOM),
                _ptrs([t.ptr for t in o["rm"]]), _ptrs([t.ptr for t in o["rv"]]), _ptrs([t.ptr for t in o["cnt"]]),
                o["out"].data, o["out"].stride if out_stride is None else out_stride, _ptrs([t.ptr for t in o["mean"]]), _ptrs([t.ptr for t in o["rstd"]]),
                _ptrs([t.ptr for t in self.part]), self.R, _ints(phases), _ACT[act]]
        if self.next is None:
            return _call("maf_bn_sum_forward", *args, _stream())
        return _call("maf_bn_sum_forward_stats", *args, self.next.ptr, self.R, nphase, _stream())

    def scratch(self):
        return self.part + ([self.next] if self.next is not None else [])


def _spread(total, n):
    """an exact integer-valued per-channel sum [C] (fp64) as n integer-valued fp32 rows that add up to it"""
    share = torch.trunc(total / n)
    rows = [share.clone() for _ in range(n - 1)] + [total - share * (n - 1)]
    return torch.stack(rows).float()


def _run_forward(name):
    if (name, "fwd") in _DONE:
        return
    c = R.BY_NAME[name]
    nb, M, Cc, dtype, act = c["nb"], c["M"], c["C"], c["dtype"], c["act"]
    inp, ref = R.forward_inputs(name), R.forward_reference(name)
    f = _Fwd(nb, dtype, M, Cc, c["R"], inp, c["idx"], stats=c["stats"])
    rk = R.replicas(Cc, c["R"])
    p0 = c["idx"] % 2
    for j in range(nb):
        f.part[j].val()[(1 - p0) * f.half:(2 - p0) * f.half] = GARBAGE              # the half the first call clears
    entry = "maf_bn_sum_forward_stats" if c["stats"] else "maf_bn_sum_forward"
    first = None
    for step, phase in enumerate((p0, 1 - p0, p0)):
        tag = "%s fwd call %d" % (name, step)
        for j in range(nb):
            if step == 0:                                                           # the exact sums, over the replicas the kernel reads: [r][2][C]
                blk = torch.stack([_spread(ref["sum_z"][j], rk), _spread(ref["sum_zz"][j], rk)], 1)
                f.part[j].val()[phase * f.half:phase * f.half + rk * 2 * Cc] = blk.reshape(-1).to(DEV)
            else:                                                                   # maf_bn_stats adds into the half the call before cleared
                assert _call("maf_bn_stats", f.z[j].data, f.z[j].stride, M, Cc, _LDT[dtype], f.part[j].ptr, c["R"], phase, _stream()) == 0, tag
        held = [p.val()[phase * f.half:(phase + 1) * f.half].clone() for p in f.part[:nb]]
        nphase = (c["idx"] // 2 + step) % 2
        if f.next is not None:
            pre_next = torch.full((2 * f.nhalf,), GARBAGE)
            pre_next[nphase * f.nhalf:(nphase + 1) * f.nhalf] = 0
            pre_next[nphase * f.nhalf:nphase * f.nhalf + 2 * Cc] = torch.arange(2 * Cc) % 5      # replica 0 is not empty: the pass ADDS
            f.next.set(pre_next)
        o = f.outputs()
        assert f.call(o, [phase] * nb, act, inp["eps"], nphase) == 0, (tag, lib.load().maf_last_error().decode())
        o["out"].assert_rest_untouched(tag + " out")
        got = o["out"].got().reshape(M, Cc)
        if c["fwd"] == "unit":
            _assert_exact(got, ref["out"].to(dtype).to(DEV), tag + " out")
        else:
            e, lim = bn_ref.err_max(got, ref["out"]), bn_ref.BARS[dtype]["y"]
            print("BNSUM %s | out %.3e (bar %.0e)" % (tag, e, lim))
            assert bool(torch.isfinite(got).all()) and _bar(entry, "out %s" % R.DTN[dtype], e, lim) <= 1, (tag, e, lim)
        if first is None:
            first = got.clone()
        else:
            _assert_exact(got, first, tag + " out against the first call's")
        for j in range(nb):
            t = "%s branch %d" % (tag, j)
            for k in ("mean", "rstd", "rm", "rv", "cnt"):
                o[k][j].assert_guards(t + " " + k)
            _assert_exact(o["mean"][j].val(), ref["mean"][j].float().to(DEV), t + " save_mean")
            _within_ulp(o["rstd"][j].val(), ref["rstd"][j], t + " save_rstd")
            _within_ulp(o["rm"][j].val(), ref["running_mean"][j], t + " running_mean")
            _within_ulp(o["rv"][j].val(), ref["running_var"][j], t + " running_var")
            assert int(o["cnt"][j].val()[0]) == 41 + j + 1, t + " num_batches_tracked"
            f.part[j].assert_guards(t + " scratch")
            p = f.part[j].val()
            assert not bool(p[(1 - phase) * f.half:(2 - phase) * f.half].any()), t + ": the other half of the scratch is not zero"
            assert torch.equal(p[phase * f.half:(phase + 1) * f.half], held[j]), t + ": the half that held the sums was written"
            assert not bool(held[j][rk * 2 * Cc:].any()), t + ": sums beyond the replicas the kernel reads"
            for k in ("gamma", "beta"):
                f.vec[k][j].assert_untouched(t + " " + k)
        if f.next is not None:
            f.next.assert_guards(tag + " next scratch")
            nk = R.replicas(Cc, c["R"])
            now, was = f.next.val().double().cpu(), pre_next.double()
            oth = slice((1 - nphase) * f.nhalf, (2 - nphase) * f.nhalf)
            assert torch.equal(now[oth], was[oth]), tag + ": the next BatchNorm's other half was written"
            lo = nphase * f.nhalf
            assert torch.equal(now[lo + nk * 2 * Cc:lo + f.nhalf], was[lo + nk * 2 * Cc:lo + f.nhalf]), tag + ": next scratch beyond its replicas was written"
            gain = (now[lo:lo + nk * 2 * Cc] - was[lo:lo + nk * 2 * Cc]).view(nk, 2, Cc).sum(0)
            stored = got.double().cpu()
            want = torch.stack([stored.sum(0), (stored ** 2).sum(0)])
            if c["fwd"] == "unit":
                assert torch.equal(gain, want), "%s: the next BatchNorm's sums differ from those of the stored out by %g" % (tag, float((gain - want).abs().max()))
            else:
                lim = bn_ref.BARS[dtype]["stat"]
                for w, nm in enumerate(("sum out", "sum out^2")):
                    e = bn_ref.err_max(gain[w], want[w])
                    print("BNSUM %s | STATS %s %.3e (bar %.0e)" % (tag, nm, e, lim))
                    assert _bar(entry, "%s %s" % (nm, R.DTN[dtype]), e, lim) <= 1, (tag, nm, e, lim)
    _DONE.add((name, "fwd"))


@pytest.mark.parametrize("name", R.names())
def test_forward(name):
    _run_forward(name)


# ------------------------------------------------------------------------------------------------------------------------------------------ refusals
def _refusal_inputs(r, nalloc):
    M, dtype = 2, r["dtype"]
    n = R.NGRP[dtype]
    Cb = -(-r["C"] // n) * n                                                        # the buffers are laid out for the next whole group
    g = torch.Generator().manual_seed(r["C"])
    z = [torch.randint(-4, 5, (M, Cb), generator=g).to(dtype) for _ in range(nalloc)]
    vec = [torch.ones(Cb) for _ in range(nalloc)]
    return Cb, dict(z=z, dy=z[0], gamma=vec, beta=vec, mean=vec, rstd=vec, pre_dgamma=vec, pre_dbeta=vec, running_mean=vec, running_var=vec)


@pytest.mark.parametrize("r", R.REFUSED, ids=[r["tag"] for r in R.REFUSED])
def test_refused_calls_touch_nothing(r):
    """nb 1 / 5, C off the channel group, a misaligned stride, C > 4096, a bad phase (MAF_E_ARG) and one channel group past the (nb, C) limit of every nb and dtype
    (MAF_E_UNSUPPORTED) — in both directions: the code, and every output and scratch buffer bit-identical afterwards (both scratch halves hold garbage)."""
    if (r["tag"], "refused") in _DONE:
        return
    want = -2 if r.get("unsupported") else -1
    na = max(r["nb"], 2)
    Cb, inp = _refusal_inputs(r, na)
    bad = r.get("bad")
    b = _Bwd(r["nb"], r["dtype"], 2, Cb, 16, inp, 0, nalloc=na)
    b.part.set(torch.full((2 * b.half,), GARBAGE))
    outs = b.outputs()
    rc = b.call(outs, 2 if bad == "phase" else 0, 1, None, Cc=r["C"], dy_stride=b.dy.stride + 1 if bad == "stride" else None)
    assert rc == want, (r["tag"], "backward", rc, lib.load().maf_last_error().decode())
    for j in range(na):
        outs[0][j].assert_unwritten(r["tag"] + " dz")
        outs[1][j].assert_untouched(r["tag"] + " dgamma"), outs[2][j].assert_untouched(r["tag"] + " dbeta")
    b.part.assert_untouched(r["tag"] + " bpart")
    for stats in (False, True):
        f = _Fwd(r["nb"], r["dtype"], 2, Cb, 16, inp, 0, nalloc=na, stats=stats)
        for p in f.scratch():
            p.set(torch.full((p.n,), GARBAGE))
        o = f.outputs()
        rc = f.call(o, [2 if bad == "phase" else 0] * na, None, R.EPS, 0, Cc=r["C"], out_stride=o["out"].stride + 1 if bad == "stride" else None)
        assert rc == want, (r["tag"], "forward", stats, rc, lib.load().maf_last_error().decode())
        o["out"].assert_unwritten(r["tag"] + " out")
        for k in ("mean", "rstd", "rm", "rv", "cnt"):
            for t in o[k]:
                t.assert_untouched(r["tag"] + " " + k)
        for p in f.scratch():
            p.assert_untouched(r["tag"] + " scratch")
    _DONE.add((r["tag"], "refused"))


def test_python_gate_sends_the_refused_widths_to_the_bn_act_chain():
    """train_ops.bn_sum's gate is the library's rule: the largest accepted width of every nb takes the merged kernel, one channel group more takes the bn_act chain
    (and does not raise); both give finite sums of the right shape."""
    from maf_yolo_amd import train_ops
    for nb in (2, 3, 4):
        for dtype in (F16, F32):
            top = R.max_c(nb, dtype)
            for Cc, merged in ((top, True), (top + R.NGRP[dtype], False)):
                assert train_bn.bn_sum_takes(nb, Cc) == merged == R.takes(nb, Cc)
                g = torch.Generator().manual_seed(Cc)
                zs = [torch.randn(1, Cc, 1, 2, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(nb)]
                bns = [torch.nn.BatchNorm2d(Cc, eps=1e-3, momentum=0.03).to(DEV).train() for _ in range(nb)]
                n0 = train_ops.stats.get("native_bn_sum", 0)
                y = train_ops.bn_sum(zs, bns)
                torch.cuda.synchronize()
                assert train_ops.stats.get("native_bn_sum", 0) == n0 + (1 if merged else 0), (nb, Cc)
                assert y.shape == zs[0].shape and bool(torch.isfinite(y).all())


# ------------------------------------------------------------------------------------------------------------------------------------------ the tally
def test_every_case_ran_and_the_tally_is_the_expected_one():
    """Runs whatever case has not run yet, then: the accepted and refused launches per entry point are exactly what the case lists imply — a case silently skipped
    fails the file.  Prints the tally and the largest err / bar for the docstring."""
    for c in R.CASES:
        for fam in ("E", "B"):
            if fam in c["bwd"]:
                _run_backward(c["name"], fam)
        _run_forward(c["name"])
    for r in R.REFUSED:
        test_refused_calls_touch_nothing(r)
    for entry, (a, n) in sorted(TALLY.items()):
        print("TALLY %-28s accepted %4d  refused %3d" % (entry, a, n))
    for (entry, name), r in sorted(WORST.items()):
        print("WORST %-28s %-20s %.4f" % (entry, name, r))
    nE, nB = len(R.names(lambda c: "E" in c["bwd"])), len(R.names(lambda c: "B" in c["bwd"]))
    nS, nF = len(R.names(lambda c: c["stats"])), len(R.names(lambda c: not c["stats"]))
    assert TALLY["maf_bn_sum_backward"] == [3 * nE + nB, len(R.REFUSED)], TALLY
    assert TALLY["maf_bn_sum_forward"] == [3 * nF, len(R.REFUSED)], TALLY
    assert TALLY["maf_bn_sum_forward_stats"] == [3 * nS, len(R.REFUSED)], TALLY
    assert TALLY["maf_bn_stats"] == [2 * sum(c["nb"] for c in R.CASES), 0], TALLY
