"""The merged BatchNorm sum of csrc/bn_sum.hip (out = act(sum_j BN_j(z_j)), its backward) restated in plain fp64 torch on the CPU, the cases of
tests/test_gpu_bn_sum_edges.py, and the launcher's grid / slice / replica arithmetic recomputed in Python so that every case can show it reaches the branch it names
(tests/test_bn_sum_ref_host.py checks all of that on the very tensors the GPU test uses).

    xhat_j = (z_j - mean_j) * rstd_j        u = sum_j (xhat_j * gamma_j + beta_j)        out = act(u)        g = dy * [u > 0] (ReLU) or dy
    dbeta_j = sum g        dgamma_j = sum g * xhat_j        dz_j = gamma_j * rstd_j * (g - mean(g) - xhat_j * mean(g * xhat_j))

Families of inputs:
    E    backward, exact: mean = 0 and rstd = 1 are ARGUMENTS of the backward; gamma in {+-0.5, +-1, +-2}, beta in halves, z and dy integers in [-4, 4].  xhat, u, g and
         every partial sum are exact in fp32 in any order: dgamma / dbeta bit for bit for every M, dz bit for bit for M a power of two (mean(.) is a dyadic
         rational with fewer than 24 bits); u == 0 is hit exactly, where the ReLU's g is 0.
    B    backward, real-valued: bn_ref.ladder_rows at (0.4, 1.7), mean / rstd the fp64 moments rounded to fp32 (what the kernel reads); bn_ref.BARS.  With ReLU, dy is
         zeroed wherever |u| < 2^-12 * sum_j (|xhat_j gamma_j| + |beta_j|): the mask is then not a matter of rounding (at most 1 % of a case's elements).
    int  forward: integer z in [-4, 4] (sums of z and z^2 exact in fp32), eps = 1e-3; out within bn_ref.BARS.
    unit forward, exact: z = +-1 with as many of each per channel (mean 0, variance 1), eps = 3 so that rstd = 0.5 exactly, gamma in {+-2, +-4}, beta integers: `out`
         is an integer, torch.equal, and the STATS form's {sum out, sum out^2} are exact."""
import functools

import torch

import bn_ref
from wgrad_ref import int_case

F16, F32 = torch.float16, torch.float32
NGRP = {F16: 8, F32: 4}                                        # elements of a 16-byte channel group
DTN = {F16: "fp16", F32: "fp32"}
MAX_LDS = 160 * 1024                                           # bn_sum.hip: kMaxLds
K_U = 2                                                        # bn_sum.hip: kU
EPS = float(torch.tensor(1e-3, dtype=F32))                     # the float the kernel is handed, as a double
MOM = float(torch.tensor(0.03, dtype=F32))


# ------------------------------------------------------------------------------------------------ the launcher's arithmetic (csrc/bn_sum.hip)
def takes(nb, C):
    """check(): the (nb, C) both directions launch"""
    return 2 <= nb <= 4 and 0 < C <= 4096 and (2 + 5 * nb) * C * 4 <= MAX_LDS


def max_c(nb, dtype):
    n = NGRP[dtype]
    return min(4096, MAX_LDS // ((2 + 5 * nb) * 4)) // n * n


def replicas(C, R):
    want = max(1024 // C, 1)
    return min(R, want, 16)


def apply_geom(M, C, dtype):
    """apply_grid() and the lane map of both apply kernels"""
    groups = C // NGRP[dtype]
    gpb = min(groups, 256)
    plan = 256 // gpb
    ppl_small = 8 if M * C <= 7000000 else 16
    g = -(-M // (plan * 16))
    ppl = 8
    while g < 1024 and ppl >= ppl_small:
        g = -(-M // (plan * ppl))
        ppl >>= 1
    g = max(1, min(8192, g))
    return dict(groups=groups, gpb=gpb, plan=plan, grid=g, chunk=-(-M // g), passes=-(-groups // gpb), big=ppl_small == 16)


def stats_geom(M, C, dtype):
    """stats_grid() and the lane map of bn_sum_bwd_stats_kernel"""
    groups = C // NGRP[dtype]
    nslice = -(-groups // 8)
    gs = -(-groups // nslice)
    plan = 256 // gs
    gx = -(-M // (plan * 32))
    ppl_small = 8 if M * C <= 7000000 else 16
    ppl = 16
    while gx * nslice < 1024 and ppl >= ppl_small:
        gx = -(-M // (plan * ppl))
        ppl >>= 1
    gx = max(1, min(4096, gx))
    return dict(groups=groups, nslice=nslice, gs=gs, plan=plan, gx=gx, chunk=-(-M // gx), wave=(gs & (gs - 1)) == 0, short_last=groups - (nslice - 1) * gs < gs)


# ------------------------------------------------------------------------------------------------ the cases
CASES = []


def _case(tag, why, nb, dtype, act, C, M, R=16, acc=0, bwd="E", fwd="int", stats=False):
    name = "%s nb%d %s %s C%d M%d R%d acc%d" % (tag, nb, DTN[dtype], act or "none", C, M, R, acc)
    CASES.append(dict(name=name, tag=tag, why=why, nb=nb, dtype=dtype, act=act, C=C, M=M, R=R, acc=acc, bwd=bwd, fwd=fwd, stats=stats, idx=len(CASES)))


GROUPS = [(1, "1 group: the wave-shuffle path, 256 pixel lanes"), (2, "2 groups: wave shuffle"), (4, "4 groups: wave shuffle"), (8, "8 groups: one full slice, wave shuffle"),
          (3, "3 groups: the LDS parking path"), (5, "5 groups: LDS parking"), (6, "6 groups: LDS parking"), (7, "7 groups: LDS parking"),
          (9, "9 groups: two slices of 5, the last one short, LDS parking")]
_RS = (16, 1, 64)


def _m_edges(C, dtype):
    """(M, why) for a width: 1, 2, around kU * plan of the apply kernels (one workgroup), a ragged chunk over two workgroups, powers of two"""
    p = apply_geom(1, C, dtype)["plan"]
    return [(1, "M 1"), (2, "M 2"), (K_U * p - 1, "M one below kU * plan: the unroll tail alone"), (K_U * p, "M = kU * plan: one unrolled trip, no tail"),
            (K_U * p + 1, "M one above kU * plan: one trip and a tail of one"), (8 * p + 5, "M = 8 plan + 5: two workgroups, the last chunk shorter"),
            (256, "M 256: a power of two, dz exact"), (4096, "M 4096: a power of two over several workgroups, dz exact")]


def _build():
    k = 0
    for gi, (g, gwhy) in enumerate(GROUPS):
        for di, dtype in enumerate((F16, F32)):
            C = g * NGRP[dtype]
            for mi, (M, mwhy) in enumerate(_m_edges(C, dtype)):
                nb = 2 + k % 3                                                     # k % 6: the six (nb, act) pairs in turn, under both dtypes of every width
                act = "relu" if (k // 3) % 2 else None
                # the ragged two-workgroup M also runs family B; the exact "unit" forward (with the STATS form) at the even M of every other width
                unit = M % 2 == 0 and (gi + mi) % 2 == 0 and C // NGRP[dtype] <= 256
                _case("groups", gwhy + "; " + mwhy, nb, dtype, act, C, M, R=_RS[(k // 2) % 3], acc=(k // 6 + gi) % 2, bwd="EB" if mi == 5 else "E", fwd="unit" if unit else "int", stats=unit)
                k += 1
    # more than 256 channel groups: the second trip of the g0 loop (gpb 256, plan 1; the second trip holds ONE group)
    _case("g0", "257 groups: the second pass of the g0 loop (fp16)", 3, F16, "relu", 2056, 2, R=16, acc=1, bwd="E")
    _case("g0", "257 groups: the second pass of the g0 loop (fp16), three pixels, family B", 2, F16, None, 2056, 3, R=1, acc=0, bwd="EB")
    _case("g0", "257 groups: the second pass of the g0 loop (fp32)", 4, F32, None, 1028, 2, R=64, acc=0, bwd="E")
    _case("g0", "257 groups: the second pass of the g0 loop (fp32), three pixels, family B", 3, F32, "relu", 1028, 3, R=16, acc=1, bwd="EB")
    # the other grid rule
    _case("big", "M * C = 8 388 608 > 7 000 000: 16 pixels per lane in both grids", 2, F16, "relu", 64, 131072, R=16, acc=1, bwd="E", fwd="unit", stats=True)
    # a STATS form whose `out` is not an integer: family B, BARS['stat']
    _case("stats", "STATS form on real-valued sums: 9 groups, several workgroups", 3, F16, None, 72, 685, R=16, acc=0, bwd="B", fwd="int", stats=True)
    _case("stats", "STATS form on real-valued sums, fp32, ReLU", 2, F32, "relu", 24, 1029, R=16, acc=0, bwd="B", fwd="int", stats=True)
    # both sides of the (nb, C) limit: the largest accepted width, for values
    for nb in (2, 3, 4):
        for dtype in (F16, F32):
            _case("limit", "the largest C both directions launch for nb %d: (2 + 5 nb) C floats <= 160 KiB" % nb, nb, dtype, "relu" if nb % 2 else None, max_c(nb, dtype), 2,
                  R=16, acc=nb % 2, bwd="E")


_build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# refused calls: (tag, nb, dtype, C, what is wrong) — `bad` names the argument the test spoils
REFUSED = [dict(tag="nb 1", nb=1, dtype=F16, C=16), dict(tag="nb 5", nb=5, dtype=F16, C=16),
           dict(tag="C not a multiple of the group (fp16)", nb=2, dtype=F16, C=12), dict(tag="C not a multiple of the group (fp32)", nb=3, dtype=F32, C=6),
           dict(tag="a stride not a multiple of the group", nb=2, dtype=F16, C=16, bad="stride"),
           dict(tag="C > 4096", nb=2, dtype=F16, C=4104), dict(tag="a bad phase", nb=3, dtype=F32, C=8, bad="phase")]
for _nb in (2, 3, 4):
    for _dt in (F16, F32):
        REFUSED.append(dict(tag="one group past the limit of nb %d %s" % (_nb, DTN[_dt]), nb=_nb, dtype=_dt, C=max_c(_nb, _dt) + NGRP[_dt], unsupported=True))


def names(pred=None):
    return [c["name"] for c in CASES if pred is None or pred(c)]


# ------------------------------------------------------------------------------------------------ inputs
_GAMMA_E = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
_GAMMA_U = torch.tensor([2.0, -2.0, 4.0, -4.0])


def _gen(c, salt):
    return torch.Generator().manual_seed(1000 * c["idx"] + salt)


@functools.lru_cache(maxsize=None)
def backward_inputs(name, fam):
    """dict: z [nb] x [M, C], dy [M, C] (case dtype), gamma / beta / mean / rstd [nb] x [C] fp32, pre_dgamma / pre_dbeta [nb] x [C] fp32, zeroed (family B, ReLU: the
    fraction of dy set to 0 next to the kink)"""
    c = BY_NAME[name]
    nb, M, C, dtype = c["nb"], c["M"], c["C"], c["dtype"]
    g = _gen(c, 1 if fam == "E" else 2)
    out = dict(zeroed=0.0)
    if fam == "E":
        out["z"] = [int_case((M, C), g, amp=4).to(dtype) for _ in range(nb)]
        out["dy"] = int_case((M, C), g, amp=4).to(dtype)
        out["gamma"] = [_GAMMA_E[torch.randint(0, 6, (C,), generator=g)] for _ in range(nb)]
        out["beta"] = [torch.randint(-4, 5, (C,), generator=g).float() / 2 for _ in range(nb)]
        out["mean"] = [torch.zeros(C) for _ in range(nb)]
        out["rstd"] = [torch.ones(C) for _ in range(nb)]
        out["pre_dgamma"] = [torch.randint(-64, 65, (C,), generator=g).float() / 2 for _ in range(nb)]
        out["pre_dbeta"] = [torch.randint(-64, 65, (C,), generator=g).float() / 2 for _ in range(nb)]
    else:
        out["z"] = [bn_ref.ladder_rows(M, C, 0.4, 1.7, dtype, 1000 * c["idx"] + 10 + j) for j in range(nb)]
        dy = torch.randn(M, C, generator=g).to(dtype)
        out["gamma"] = [torch.rand(C, generator=g) + 0.5 for _ in range(nb)]
        out["beta"] = [torch.randn(C, generator=g) * 0.3 for _ in range(nb)]
        mv = [bn_ref.moments(z) for z in out["z"]]
        out["mean"] = [m.float() for m, _ in mv]
        out["rstd"] = [(1.0 / torch.sqrt(v + EPS)).float() for _, v in mv]
        out["pre_dgamma"] = [torch.randn(C, generator=g) for _ in range(nb)]
        out["pre_dbeta"] = [torch.randn(C, generator=g) for _ in range(nb)]
        if c["act"] == "relu":
            xh = [(z.double() - m.double()) * r.double() for z, m, r in zip(out["z"], out["mean"], out["rstd"])]
            u = sum(x * ga.double() + be.double() for x, ga, be in zip(xh, out["gamma"], out["beta"]))
            scale = sum((x * ga.double()).abs() + be.double().abs() for x, ga, be in zip(xh, out["gamma"], out["beta"]))
            near = u.abs() < 2.0 ** -12 * scale
            dy = torch.where(near, torch.zeros_like(dy), dy)
            out["zeroed"] = float(near.double().mean())
        out["dy"] = dy
    return out


@functools.lru_cache(maxsize=None)
def forward_inputs(name):
    """dict: z, gamma, beta as above; eps; running_mean / running_var [nb] x [C] fp32 on entry"""
    c = BY_NAME[name]
    nb, M, C, dtype = c["nb"], c["M"], c["C"], c["dtype"]
    g = _gen(c, 3)
    out = {}
    if c["fwd"] == "unit":
        assert M % 2 == 0
        zs = []
        for _ in range(nb):
            order = torch.argsort(torch.rand(M, C, generator=g), dim=0)
            zs.append(torch.where(order < M // 2, 1.0, -1.0).to(dtype))
        out["z"], out["eps"] = zs, 3.0
        out["gamma"] = [_GAMMA_U[torch.randint(0, 4, (C,), generator=g)] for _ in range(nb)]
        out["beta"] = [torch.randint(-2, 3, (C,), generator=g).float() for _ in range(nb)]
    else:
        out["z"], out["eps"] = [int_case((M, C), g, amp=4).to(dtype) for _ in range(nb)], EPS
        out["gamma"] = [_GAMMA_E[torch.randint(0, 6, (C,), generator=g)] for _ in range(nb)]
        out["beta"] = [torch.randint(-4, 5, (C,), generator=g).float() / 2 for _ in range(nb)]
    out["running_mean"] = [torch.randn(C, generator=g) * 0.5 for _ in range(nb)]
    out["running_var"] = [torch.rand(C, generator=g) + 0.5 for _ in range(nb)]
    return out


# ------------------------------------------------------------------------------------------------ the reference
def sum_ref(zs, gammas, betas, means, rstds, act, dtype, dy=None):
    """fp64 on the stored values; dict out, u [, dz [nb], dgamma [nb], dbeta [nb]]"""
    xh = [(z.double() - m.double()) * r.double() for z, m, r in zip(zs, means, rstds)]
    u = sum(x * ga.double() + be.double() for x, ga, be in zip(xh, gammas, betas))
    res = dict(u=u, out=bn_ref.store(torch.clamp(u, min=0) if act == "relu" else u, dtype))
    if dy is not None:
        g = dy.double() * (u > 0).double() if act == "relu" else dy.double()
        res["dbeta"] = [g.sum(0) for _ in zs]
        res["dgamma"] = [(g * x).sum(0) for x in xh]
        res["dz_exact"] = [ga.double() * r.double() * (g - g.mean(0) - x * (g * x).mean(0)) for x, ga, r in zip(xh, gammas, rstds)]
        res["dz"] = [bn_ref.store(t, dtype) for t in res["dz_exact"]]
    return res


@functools.lru_cache(maxsize=None)
def backward_reference(name, fam):
    c = BY_NAME[name]
    i = backward_inputs(name, fam)
    return sum_ref(i["z"], i["gamma"], i["beta"], i["mean"], i["rstd"], c["act"], c["dtype"], i["dy"])


@functools.lru_cache(maxsize=None)
def forward_reference(name):
    """dict out, mean / var / rstd / running_mean / running_var [nb] (fp64), sum_z / sum_zz [nb] (the exact sums, fp64)"""
    c = BY_NAME[name]
    i = forward_inputs(name)
    M = c["M"]
    mv = [bn_ref.moments(z) for z in i["z"]]
    mean, var = [m for m, _ in mv], [v for _, v in mv]
    rstd = [1.0 / torch.sqrt(v + i["eps"]) for v in var]
    res = sum_ref(i["z"], i["gamma"], i["beta"], mean, rstd, c["act"], c["dtype"])
    res.update(mean=mean, var=var, rstd=rstd)
    res["running_mean"] = [(1 - MOM) * rm.double() + MOM * m for rm, m in zip(i["running_mean"], mean)]
    res["running_var"] = [(1 - MOM) * rv.double() + MOM * (v * M / (M - 1) if M > 1 else v) for rv, v in zip(i["running_var"], var)]
    res["sum_z"] = [z.double().sum(0) for z in i["z"]]
    res["sum_zz"] = [(z.double() ** 2).sum(0) for z in i["z"]]
    return res


def ulp32(t):
    """the spacing of fp32 at |t| (fp64 tensor), normal range"""
    return torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -126))) - 23)


def is_pow2(M):
    return M & (M - 1) == 0
