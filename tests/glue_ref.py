"""The structural kernels of the train graph — max-pool, nearest 2x upsample, the detect join, the NHWC sum, the column sum (csrc/pool_train.hip, csrc/detect_join.hip,
csrc/train_ops.hip) — restated in plain fp64 torch on the CPU, with the cases of tests/test_gpu_glue_edges.py and the launchers' grid arithmetic recomputed in Python
(tests/test_glue_ref_host.py checks the references and that every case reaches the branch it names, on the very tensors the GPU test uses).

Everything here is a move, a maximum or a short sum of small integers: every result is held bit for bit, except the detect join's sigmoid and its derivative, which
are held to a bound in ulps of the fp64 value.  All tensors are NHWC: [B, H, W, C] (the join: [B, pixels, C] per level)."""
import functools

import torch
import torch.nn.functional as F

from wgrad_ref import int_case

F16, F32 = torch.float16, torch.float32
NGRP = {F16: 8, F32: 4}
DTN = {F16: "fp16", F32: "fp32"}
NEG = float("-inf")
NAN = float("nan")


def _gen(salt):
    return torch.Generator().manual_seed(salt)


# ------------------------------------------------------------------------------------------------ max-pool
POOL = []


def _pool(why, k, s, p, B, H, W, C, dtype=F16, fill="ties"):
    POOL.append(dict(name="pool k%d s%d p%d %dx%dx%dx%d %s %s" % (k, s, p, B, H, W, C, DTN[dtype], fill), why=why, k=k, s=s, p=p, B=B, H=H, W=W, C=C, dtype=dtype, fill=fill, idx=len(POOL)))


_pool("MP of MPRep; a 5 x 7 map the stride does not divide: the last row and column belong to no window, dx = 0 there", 2, 2, 0, 2, 5, 7, 16)
_pool("(3, 1, 1) over several channel groups, fp32", 3, 1, 1, 2, 6, 5, 12, F32)
_pool("SPPF's pool on an odd map", 5, 1, 2, 1, 7, 9, 8)
_pool("(3, 2, 1): nh % stride picks every other output; 6 x 7", 3, 2, 1, 2, 6, 7, 24)
_pool("(2, 1, 1): the output is larger than the input", 2, 1, 1, 1, 4, 5, 8, F32)
_pool("(4, 3, 2): stride 3, an even window, the largest padding (2 pad == k); 9 x 8: the last windows hang over the map", 4, 3, 2, 2, 9, 8, 8)
_pool("(7, 2, 3) on 10 x 9", 7, 2, 3, 1, 10, 9, 16, F32)
_pool("(15, 1, 7): the largest window, argmax up to 224 in one byte", 15, 1, 7, 1, 9, 16, 8)
_pool("(15, 15, 0) on 17 x 31: one row of two windows, rows 15-16 and column 30 in no window", 15, 15, 0, 2, 17, 31, 8)
_pool("a 1 x 1 map under (3, 1, 1): the window is its centre alone", 3, 1, 1, 3, 1, 1, 8)
_pool("H + 2 pad == k: one output row (5, 1, 2 on 1 x 6)", 5, 1, 2, 1, 1, 6, 8, F32)
_pool("H + 2 pad == k and W + 2 pad == k: (7, 2, 3) on 1 x 1", 7, 2, 3, 2, 1, 1, 16)
_pool("H + 2 pad == k under the largest window: (15, 1, 7) on 1 x 3", 15, 1, 7, 1, 1, 3, 8)
_pool("255 threads in both directions: one below a multiple of 256", 3, 1, 1, 1, 15, 17, 8)
_pool("257 threads in both directions: one above a multiple of 256", 3, 1, 1, 1, 1, 257, 4, F32)
_pool("a -inf pixel, windows of -inf alone (the first in-image element is kept), NaN pixels (a later NaN replaces an earlier one)", 3, 1, 1, 2, 6, 6, 8, F16, "special")
_pool("the same under a stride: all -inf / NaN windows with (2, 2, 0), fp32", 2, 2, 0, 1, 6, 8, 4, F32, "special")
_pool("the same with padding and stride: (3, 2, 1)", 3, 2, 1, 1, 7, 7, 8, F16, "special")
POOL_BY = {c["name"]: c for c in POOL}

POOL_REFUSED = [("k 1", dict(k=1, s=1, p=0)), ("k 16", dict(k=16, s=1, p=8, H=20, W=20)), ("stride > k", dict(k=2, s=3, p=0)), ("2 pad > k", dict(k=3, s=1, p=2)),
                ("a window larger than the padded map", dict(k=7, s=1, p=1, H=4, W=9)), ("misaligned C", dict(C=12)), ("a misaligned source stride", dict(bump_x=1)),
                ("a misaligned output stride", dict(bump_y=1))]


def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def pool_inputs(name):
    c = POOL_BY[name]
    g = _gen(100 + c["idx"])
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    x = torch.randint(0, 3, (B, H, W, C), generator=g).to(c["dtype"])                  # three values: ties in almost every window
    if c["fill"] == "special":
        x[:, :3, :4] = NEG                                                             # a block of -inf: windows of -inf alone
        x[:, 4, 1] = NEG                                                               # a lone -inf pixel
        x[:, 4:6, 4] = NAN                                                             # two NaN pixels in one column: windows holding two
        x[:, 3, 5, : C // 2] = NAN                                                     # ... and one that is NaN in half of the channels
    Ho, Wo = pool_out(H, c["k"], c["s"], c["p"]), pool_out(W, c["k"], c["s"], c["p"])
    dy = int_case((B, Ho, Wo, C), g, amp=3).to(c["dtype"])
    return dict(x=x, dy=dy)


def pool_ref(x, dy, k, s, p):
    """(y, idx uint8 [window row * k + column], dx) of NHWC x / dy, by F.max_pool2d(return_indices=True) in fp64 and its autograd"""
    B, H, W, C = x.shape
    xn = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y, flat = F.max_pool2d(xn, k, s, p, return_indices=True)
    Ho, Wo = y.shape[2], y.shape[3]
    y.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    ih, iw = flat // W, flat % W
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    row, col = ih - (oh * s - p), iw - (ow * s - p)
    assert bool(((row >= 0) & (row < k) & (col >= 0) & (col < k)).all())
    idx = (row * k + col).to(torch.uint8)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return nhwc(y), nhwc(idx), nhwc(xn.grad)


@functools.lru_cache(maxsize=None)
def pool_reference(name):
    c, i = POOL_BY[name], pool_inputs(name)
    return pool_ref(i["x"], i["dy"], c["k"], c["s"], c["p"])


def pool_threads(c):
    """threads of the forward / backward launch"""
    cg = c["C"] // NGRP[c["dtype"]]
    return c["B"] * pool_out(c["H"], c["k"], c["s"], c["p"]) * pool_out(c["W"], c["k"], c["s"], c["p"]) * cg, c["B"] * c["H"] * c["W"] * cg


# ------------------------------------------------------------------------------------------------ upsample 2x
UP = [dict(why="B, H, W all odd, two channel groups", B=3, H=5, W=7, C=16, dtype=F16), dict(why="a 1 x 1 map, one group", B=1, H=1, W=1, C=8, dtype=F16),
      dict(why="fp32, W = 1, three groups", B=2, H=3, W=1, C=12, dtype=F32), dict(why="257 threads: one above a multiple of 256", B=1, H=1, W=257, C=4, dtype=F32),
      dict(why="255 threads: one below a multiple of 256", B=1, H=15, W=17, C=8, dtype=F16)]
for _i, _c in enumerate(UP):
    _c.update(idx=_i, name="up2 %dx%dx%dx%d %s" % (_c["B"], _c["H"], _c["W"], _c["C"], DTN[_c["dtype"]]))
UP_BY = {c["name"]: c for c in UP}
UP_REFUSED = [("misaligned C", dict(C=12)), ("a misaligned source stride", dict(bump_x=1)), ("a misaligned output stride", dict(bump_y=1)), ("B 0", dict(B=0))]


@functools.lru_cache(maxsize=None)
def up_inputs(name):
    c = UP_BY[name]
    g = _gen(200 + c["idx"])
    return dict(x=int_case((c["B"], c["H"], c["W"], c["C"]), g, amp=9).to(c["dtype"]), dy=int_case((c["B"], 2 * c["H"], 2 * c["W"], c["C"]), g, amp=3).to(c["dtype"]))


def up_ref(x, dy):
    y = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H2, W2, C = dy.shape
    dx = dy.double().view(B, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))
    return y, dx


# ------------------------------------------------------------------------------------------------ detect join
JOIN = []


def _join(why, levels, nc, nreg, B, dtype):
    JOIN.append(dict(name="join %s nc%d nreg%d B%d %s" % ("-".join(map(str, levels)), nc, nreg, B, DTN[dtype]), why=why, levels=tuple(levels), nc=nc, nreg=nreg, B=B, dtype=dtype, idx=len(JOIN)))


_join("one level of one pixel", (1,), 4, 4, 1, F16)
_join("one level of one pixel, fp32, several images", (1,), 12, 68, 3, F32)
_join("two levels", (7, 2), 12, 4, 2, F16)
_join("three levels (5, 3, 1): the model's count, odd sizes; reg 68 -> pad 72", (5, 3, 1), 80, 68, 2, F16)
_join("three levels, fp32 (no pad needed: 68 is a multiple of 4)", (5, 3, 1), 80, 68, 2, F32)
_join("four levels (64, 16, 4, 1): the most the kernel takes; 1445 threads forward", (64, 16, 4, 1), 12, 68, 1, F16)
_join("four levels, fp32, nc 4", (64, 16, 4, 1), 4, 4, 2, F32)
JOIN_BY = {c["name"]: c for c in JOIN}
JOIN_REFUSED = [("5 levels", dict(levels=(1, 1, 1, 1, 1))), ("nc % 4 != 0", dict(nc=6)), ("nreg % 4 != 0", dict(nreg=6)), ("0 levels", dict(levels=()))]


def pad_to(n, dtype):
    return -(-n // NGRP[dtype]) * NGRP[dtype]


@functools.lru_cache(maxsize=None)
def join_inputs(name):
    """cls / reg: per level [B, pixels, C]; d_cls / d_reg [B, A, C]; y [B, A, nc]: the stored probabilities the backward reads"""
    c = JOIN_BY[name]
    g = _gen(300 + c["idx"])
    dt = c["dtype"]
    cls, reg = [], []
    for hw in c["levels"]:
        t = (torch.rand(c["B"], hw, c["nc"], generator=g) * 24 - 12)
        flat = t.view(-1)
        flat[0], flat[1 % flat.numel()], flat[2 % flat.numel()] = 0.0, 12.0, -12.0      # the ends of the range and 0 in every level
        cls.append(t.to(dt))
        reg.append((torch.randn(c["B"], hw, c["nreg"], generator=g) * 3).to(dt))
    A = sum(c["levels"])
    y = torch.sigmoid(torch.cat([t.double() for t in cls], 1)).to(dt)
    return dict(cls=cls, reg=reg, y=y, d_cls=torch.randn(c["B"], A, c["nc"], generator=g).to(dt), d_reg=(torch.randn(c["B"], A, c["nreg"], generator=g) * 2).to(dt))


def ulp(t, dtype):
    """the spacing of `dtype` at |t| (fp64 tensor), subnormals included"""
    emin, bits = (-14, 10) if dtype == F16 else (-126, 23)
    e = torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -200))).clamp(min=emin)
    return torch.pow(2.0, e - bits)


@functools.lru_cache(maxsize=None)
def join_reference(name):
    """cls (fp64 sigmoid of the stored logits) and its bound; reg (the copy); d logits (fp64, from the stored y) and its bound; d reg (the copy)"""
    c, i = JOIN_BY[name], join_inputs(name)
    dt = c["dtype"]
    cls = torch.sigmoid(torch.cat([t.double() for t in i["cls"]], 1))
    cls_bound = ulp(cls, dt) * (1 if dt == F16 else 2)
    y = i["y"].double()
    dl = i["d_cls"].double() * (1 - y) * y
    dl_bound = ulp(dl, dt) + 3 * 2.0 ** -24 * dl.abs()
    return dict(cls=cls, cls_bound=cls_bound, reg=torch.cat(i["reg"], 1), dl=dl, dl_bound=dl_bound, dreg=i["d_reg"])


def split_levels(t, levels):
    """[B, A, C] -> per level [B, pixels, C]"""
    return list(torch.split(t, list(levels), 1))


# ------------------------------------------------------------------------------------------------ nhwc_sum
SUM = [dict(n=n, acc=acc, dtype=dt, M=M, C=C, idx=k, name="sum n%d acc%d %s M%d C%d" % (n, acc, DTN[dt], M, C),
            why="%d source%s, %s%s" % (n, "s" * (n > 1), "added to dst" if acc else "written", ": the copy path" if n == 1 and not acc else ""))
       for k, (n, acc, dt, M, C) in enumerate([(n, acc, dt, M, C) for n in (1, 2, 3, 4) for acc in (0, 1) for dt, M, C in ((F16, 37, 24), (F32, 85, 12))])]
SUM_BY = {c["name"]: c for c in SUM}
SUM_REFUSED = [("n 0", dict(n=0)), ("n 5", dict(n=5)), ("misaligned C", dict(C=12)), ("a misaligned source stride", dict(bump_x=1)), ("a misaligned destination stride", dict(bump_y=1))]


@functools.lru_cache(maxsize=None)
def sum_inputs(name):
    c = SUM_BY[name]
    g = _gen(400 + c["idx"])
    return dict(src=[int_case((c["M"], c["C"]), g, amp=3).to(c["dtype"]) for _ in range(c["n"])], dst=int_case((c["M"], c["C"]), g, amp=3).to(c["dtype"]))


def sum_ref(src, dst, acc):
    return sum(s.double() for s in src) + (dst.double() if acc else 0)


# ------------------------------------------------------------------------------------------------ colsum
COL_C = (1, 3, 68, 80, 85, 86, 128, 129, 255, 256)
COL_CAP = (129, 65600)                                          # (C, M): more than 1024 workgroups' worth of pixels at one slab per workgroup


def col_geom(M, C):
    """maf_colsum: slabs per workgroup, workgroups (before the cap), workgroups, the grid stride in pixels, idle lanes"""
    per = max(256 // C, 1)
    want = -(-M // (per * 64))
    nb = max(1, min(1024, want))
    return dict(per=per, want=want, nb=nb, step=nb * per, idle=256 - per * C)


def _col_ms(C):
    per = max(256 // C, 1)                                       # one workgroup for all of these: the stride is `per`
    return [(1, "M 1"), (7, "M 7"), (8 * per - 1, "one below 8 x the grid stride: the tail loop alone for the last slab"), (8 * per, "8 x the grid stride: one unrolled trip"),
            (8 * per + 1, "one above: a trip and a tail"), (64 * per + 1, "two workgroups")]


COL = []
for _ci, _C in enumerate(COL_C):
    for _mi, (_M, _w) in enumerate(dict(_col_ms(_C)).items()):
        _dt = F16 if (_ci + _mi) % 2 == 0 else F32
        COL.append(dict(name="colsum C%d M%d %s" % (_C, _M, DTN[_dt]), why="C %d: %d slab(s) per workgroup, %d idle lanes; %s" % (_C, max(256 // _C, 1), 256 - max(256 // _C, 1) * _C, _w),
                        C=_C, M=_M, dtype=_dt, idx=len(COL)))
COL.append(dict(name="colsum C%d M%d fp16 cap" % COL_CAP, why="the 1024-workgroup cap: 1025 workgroups' worth of pixels", C=COL_CAP[0], M=COL_CAP[1], dtype=F16, idx=len(COL)))
COL_BY = {c["name"]: c for c in COL}
COL_REFUSED = [("C 257", dict(C=257)), ("a stride below C", dict(stride=2)), ("M 0", dict(M=0))]


@functools.lru_cache(maxsize=None)
def col_inputs(name):
    c = COL_BY[name]
    g = _gen(500 + c["idx"])
    return dict(x=int_case((c["M"], c["C"]), g, amp=3).to(c["dtype"]), pre=torch.randint(1, 9, (c["C"],), generator=g).float())
