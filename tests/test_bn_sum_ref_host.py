"""The reference and the cases of tests/test_gpu_bn_sum_edges.py (tests/bn_sum_ref.py), checked on the CPU on the very tensors the GPU test uses: the fp64 reference
against torch's BatchNorm2d + autograd; every family-E case exact as claimed; the 1 % cap of family B; every case reaches the branch it names, by the launcher's grid,
slice and replica arithmetic recomputed in Python; the (nb, C) rule of both directions and of train_ops.bn_sum's gate."""
import pytest
import torch

import bn_ref
import bn_sum_ref as R

F16, F32 = torch.float16, torch.float32


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("nb", [2, 4])
def test_reference_matches_torch_autograd_in_fp64(nb, act):
    M, c = 333, 24
    g = torch.Generator().manual_seed(nb)
    zs = [bn_ref.ladder_rows(M, c, 0.4, 1.7, F32, 5 + j) for j in range(nb)]
    dy = torch.randn(M, c, generator=g)
    bns = [torch.nn.BatchNorm2d(c, eps=R.EPS, momentum=R.MOM).double() for _ in range(nb)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.copy_(torch.rand(c, generator=g) + 0.5); bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    xs = [bn_ref.as_nchw(z.double().contiguous()).detach().requires_grad_(True) for z in zs]
    u = sum(bn(x) for bn, x in zip(bns, xs))
    y = torch.relu(u) if act else u
    y.backward(bn_ref.as_nchw(dy.double().contiguous()))
    mv = [bn_ref.moments(z) for z in zs]
    ref = R.sum_ref(zs, [bn.weight.detach() for bn in bns], [bn.bias.detach() for bn in bns], [m for m, _ in mv], [1 / torch.sqrt(v + R.EPS) for _, v in mv], act, F32, dy)
    tol = 1e-10
    assert bn_ref.err_max(bn_ref.rows(y), ref["out"]) < tol
    for j in range(nb):
        assert bn_ref.err_max(bn_ref.rows(xs[j].grad), ref["dz"][j]) < tol
        assert bn_ref.err_max(bns[j].weight.grad, ref["dgamma"][j]) < tol and bn_ref.err_max(bns[j].bias.grad, ref["dbeta"][j]) < tol


def _fp32_exact(t):
    return bool((t.float().double() == t).all())


def test_every_family_e_case_is_exact_as_claimed():
    """xhat, u, g and the sums are integers or halves below 2^24 (exact in fp32 in any order); for M a power of two dz is an fp32 number; the ReLU cases hit u == 0,
    where g is 0."""
    kinks = 0
    for name in R.names(lambda c: "E" in c["bwd"]):
        c, i, ref = R.BY_NAME[name], R.backward_inputs(name, "E"), R.backward_reference(name, "E")
        assert all(float(m.abs().max()) == 0 for m in i["mean"]) and all(bool((r == 1).all()) for r in i["rstd"])
        for t in i["z"] + [i["dy"]]:
            assert bool((t.double() == t.double().round()).all()) and float(t.double().abs().max()) <= 4
        assert all(bool(torch.isin(ga.abs(), torch.tensor([0.5, 1.0, 2.0])).all()) for ga in i["gamma"]) and all(bool(((2 * be) == (2 * be).round()).all()) for be in i["beta"])
        assert bool(((2 * ref["u"]) == (2 * ref["u"]).round()).all()) and float(ref["u"].abs().max()) < 2 ** 10
        for t in ref["dgamma"] + ref["dbeta"]:
            assert bool((t == t.round()).all()) and float(t.abs().max()) < 2 ** 24 and _fp32_exact(t), name
        absum = i["dy"].double().abs().sum(0).max() * 4                                 # any partial sum of |g xhat| in any order
        assert float(absum) < 2 ** 24, name
        for pre, t in zip(i["pre_dgamma"] + i["pre_dbeta"], ref["dgamma"] + ref["dbeta"]):
            assert float(pre.abs().max()) > 0
        if R.is_pow2(c["M"]):
            assert all(_fp32_exact(t) for t in ref["dz_exact"]), name
        if c["act"] == "relu":
            z0 = ref["u"] == 0
            kinks += int(z0.sum())
            g = i["dy"].double() * (ref["u"] > 0)
            assert float(g[z0].abs().max() if bool(z0.any()) else 0) == 0
    assert kinks > 1000, kinks


def test_unit_forward_cases_are_integer_exact():
    for name in R.names(lambda c: c["fwd"] == "unit"):
        c, i, ref = R.BY_NAME[name], R.forward_inputs(name), R.forward_reference(name)
        assert all(float(m.abs().max()) == 0 for m in ref["mean"]) and all(bool((v == 1).all()) for v in ref["var"]) and all(bool((r == 0.5).all()) for r in ref["rstd"])
        out = ref["out"]
        assert bool((out == out.round()).all()) and float((out ** 2).sum(0).max()) < 2 ** 24 and c["stats"] and c["C"] // R.NGRP[c["dtype"]] <= 256
    for name in R.names(lambda c: c["fwd"] == "int"):
        ref = R.forward_reference(name)
        assert all(float(t.max()) < 2 ** 24 and bool((t == t.round()).all()) for t in ref["sum_zz"] + ref["sum_z"])


def test_family_b_relu_zeroes_at_most_one_percent():
    seen = 0
    for name in R.names(lambda c: "B" in c["bwd"]):
        i = R.backward_inputs(name, "B")
        assert i["zeroed"] <= 0.01, (name, i["zeroed"])
        seen += R.BY_NAME[name]["act"] == "relu"
        assert all(bool(torch.isfinite(t).all()) for t in R.backward_reference(name, "B")["dz"])
    assert seen >= 4


def test_every_case_reaches_the_branch_it_names():
    by = {}
    for c in R.CASES:
        by.setdefault(c["tag"], []).append(c)
    combos = {(c["nb"], c["dtype"], c["act"]) for c in R.CASES}
    assert combos == {(nb, dt, a) for nb in (2, 3, 4) for dt in (F16, F32) for a in (None, "relu")}
    assert {(c["nb"], c["dtype"], c["act"]) for c in R.CASES if "E" in c["bwd"] and R.is_pow2(c["M"]) and c["M"] >= 256} == combos       # ... each with an exact dz over many pixels
    assert {c["R"] for c in R.CASES} == {1, 16, 64} and {c["acc"] for c in R.CASES} == {0, 1}
    assert {(c["R"], R.replicas(c["C"], c["R"])) for c in R.CASES} >= {(1, 1), (16, 16), (64, 16), (16, 1), (64, 14)}                  # the clamp, 1024 / C and R itself
    wave, park = set(), set()
    for c in by["groups"]:
        s, a = R.stats_geom(c["M"], c["C"], c["dtype"]), R.apply_geom(c["M"], c["C"], c["dtype"])
        assert not a["big"] and a["passes"] == 1
        (wave if s["wave"] else park).add(s["groups"])
        if s["groups"] == 9:
            assert s["nslice"] == 2 and s["gs"] == 5 and s["short_last"] and not s["wave"]
        else:
            assert s["nslice"] == 1 and s["gs"] == s["groups"]
    assert wave == {1, 2, 4, 8} and park == {3, 5, 6, 7, 9}
    for dtype in (F16, F32):
        for g, _ in R.GROUPS:
            C = g * R.NGRP[dtype]
            ms = sorted(c["M"] for c in by["groups"] if c["C"] == C and c["dtype"] == dtype)
            p = 256 // g
            assert ms == sorted([1, 2, 2 * p - 1, 2 * p, 2 * p + 1, 8 * p + 5, 256, 4096]), (C, ms)
            for M in (2 * p - 1, 2 * p, 2 * p + 1):                                   # one workgroup: the chunk is M, the unrolled loop makes 0 / 1 / 1 trips
                a = R.apply_geom(M, C, dtype)
                assert a["grid"] == 1 and a["plan"] == p
            a = R.apply_geom(8 * p + 5, C, dtype)
            assert a["grid"] == 2 and a["chunk"] * 2 != 8 * p + 5                     # the last workgroup's chunk is shorter
            s = R.stats_geom(8 * p + 5, C, dtype)
            assert s["gx"] >= 2 or s["nslice"] == 2                                   # (9 groups: 51 pixel lanes per slice, one workgroup per slice at this M)
            assert R.apply_geom(4096, C, dtype)["grid"] > 1 and R.stats_geom(4096, C, dtype)["gx"] > 1
    for c in by["g0"]:
        a = R.apply_geom(c["M"], c["C"], c["dtype"])
        assert a["groups"] == 257 and a["gpb"] == 256 and a["plan"] == 1 and a["passes"] == 2 and R.takes(c["nb"], c["C"])
    assert {c["dtype"] for c in by["g0"]} == {F16, F32}
    big = [c for c in R.CASES if c["M"] * c["C"] > 7000000]
    assert len(big) == 1 and R.apply_geom(big[0]["M"], big[0]["C"], big[0]["dtype"])["big"] and big[0]["tag"] == "big" and R.is_pow2(big[0]["M"])
    assert R.stats_geom(big[0]["M"], big[0]["C"], big[0]["dtype"])["gx"] > 16 == R.replicas(big[0]["C"], big[0]["R"])      # more workgroups than replicas: the index wraps
    assert all(c["M"] * c["C"] < 700000 for c in R.CASES if c["tag"] != "big")
    assert any(c["stats"] and c["fwd"] == "int" for c in R.CASES) and any(c["stats"] and c["fwd"] == "unit" and R.apply_geom(c["M"], c["C"], c["dtype"])["grid"] > 1 for c in R.CASES)


def test_the_limit_is_one_rule_for_both_directions():
    """check(): (2 + 5 nb) C floats within 160 KiB — then the forward's nb 2 C floats are within the 64 KiB a kernel gets without asking, for every (nb, C) taken."""
    from maf_yolo_amd import train_bn
    assert (R.max_c(2, F16), R.max_c(3, F16), R.max_c(4, F16)) == (3408, 2408, 1856) and (R.max_c(2, F32), R.max_c(3, F32), R.max_c(4, F32)) == (3412, 2408, 1860)
    for nb in range(0, 7):
        for C in range(0, 4200, 4):
            assert train_bn.bn_sum_takes(nb, C) == R.takes(nb, C), (nb, C)
            if R.takes(nb, C):
                assert nb * 2 * C * 4 <= 64 * 1024 and (2 + 5 * nb) * C * 4 <= R.MAX_LDS
    lim = {(c["nb"], c["dtype"]): c["C"] for c in R.CASES if c["tag"] == "limit"}
    past = {(r["nb"], r["dtype"]): r["C"] for r in R.REFUSED if r.get("unsupported")}
    for nb in (2, 3, 4):
        for dt in (F16, F32):
            assert lim[(nb, dt)] == R.max_c(nb, dt) and R.takes(nb, lim[(nb, dt)]) and past[(nb, dt)] == lim[(nb, dt)] + R.NGRP[dt] and not R.takes(nb, past[(nb, dt)])
            assert past[(nb, dt)] <= 4096                                              # refused by the LDS rule, not by the width rule
