"""The references and cases of tests/test_gpu_glue_edges.py (tests/glue_ref.py), checked on the CPU on the very tensors the GPU test uses: the framework's max-pool
has the tie / -inf / NaN rule csrc/pool_train.hip documents (also for channels-last input) and glue_ref.pool_ref restates it in the kernel's window-local index;
every case reaches the branch it names, by the launchers' arithmetic recomputed in Python; every exact case is exact as claimed."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

F16, F32 = torch.float16, torch.float32
NEG, NAN = float("-inf"), float("nan")


def _pool1(vals, k=3, s=1, p=1, channels_last=False):
    """the centre output of a k x k window over `vals` (a k x k list): (value, flat index)"""
    x = torch.tensor(vals, dtype=torch.float64).view(1, 1, k, k).expand(1, 2, k, k).contiguous()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    y, i = F.max_pool2d(x, k, s, p, return_indices=True)
    return float(y[0, 1, k // 2, k // 2]), int(i[0, 1, k // 2, k // 2])


@pytest.mark.parametrize("channels_last", [False, True])
def test_the_framework_s_tie_inf_and_nan_rule(channels_last):
    v, i = _pool1([[1, 5, 5], [5, 2, 5], [0, 5, 1]], channels_last=channels_last)
    assert (v, i) == (5.0, 1)                                                          # the first maximum wins
    v, i = _pool1([[NEG] * 3] * 3, channels_last=channels_last)
    assert (v, i) == (NEG, 0)                                                          # a window of -inf alone keeps its first element ...
    x = torch.full((1, 2, 3, 3), NEG, dtype=torch.float64)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x
    y, idx = F.max_pool2d(x, 3, 1, 1, return_indices=True)
    assert int(idx[0, 0, 0, 0]) == 0 and int(idx[0, 1, 2, 2]) == 4                     # ... its first IN-IMAGE element: (1, 1) for the window of output (2, 2)
    v, i = _pool1([[1, NAN, 2], [3, NAN, 9], [0, 0, 0]], channels_last=channels_last)
    assert v != v and i == 4                                                           # a later NaN replaces an earlier one; nothing replaces a NaN but a NaN


def _pool_by_the_rule(x, dy, k, s, p):
    """the rule of csrc/pool_train.hip in plain loops: scan the in-image part of the window row by row; an element replaces the running maximum if it is greater, or
    NaN, or the first; dx by scattering dy to the chosen element"""
    B, H, W, C = x.shape
    Ho, Wo = R.pool_out(H, k, s, p), R.pool_out(W, k, s, p)
    xd = x.double()
    y = torch.full((B, Ho, Wo, C), NEG, dtype=torch.float64)
    idx = torch.full((B, Ho, Wo, C), -1, dtype=torch.int64)
    dx = torch.zeros(B, H, W, C, dtype=torch.float64)
    for oh in range(Ho):
        for ow in range(Wo):
            m, am = y[:, oh, ow], idx[:, oh, ow]
            for i in range(k):
                for j in range(k):
                    ih, iw = oh * s - p + i, ow * s - p + j
                    if not (0 <= ih < H and 0 <= iw < W):
                        continue
                    f = xd[:, ih, iw]
                    take = (f > m) | torch.isnan(f) | (am < 0)
                    m[take], am[take] = f[take], i * k + j
            for i in range(k):
                for j in range(k):
                    ih, iw = oh * s - p + i, ow * s - p + j
                    if 0 <= ih < H and 0 <= iw < W:
                        dx[:, ih, iw] += torch.where(am == i * k + j, dy[:, oh, ow].double(), torch.zeros(()).double())
    return y, idx.to(torch.uint8), dx


def _eq_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("name", list(R.POOL_BY))
def test_pool_reference_is_the_kernel_s_documented_rule(name):
    c, i = R.POOL_BY[name], R.pool_inputs(name)
    y, idx, dx = R.pool_reference(name)
    y2, idx2, dx2 = _pool_by_the_rule(i["x"], i["dy"], c["k"], c["s"], c["p"])
    assert _eq_nan(y, y2) and torch.equal(idx, idx2) and torch.equal(dx, dx2)
    assert int(idx.max()) < c["k"] ** 2 <= 225
    # exact in the case's dtype: y is a stored value; the gathered sums are small integers
    assert torch.equal(dx, dx.round()) and float(dx.abs().max()) <= 2048 and _eq_nan(y.to(c["dtype"]).double(), y)
    # the same through a channels-last input
    xn = i["x"].double().permute(0, 3, 1, 2)                                            # (a channels-last view of the NHWC tensor)
    assert xn.is_contiguous(memory_format=torch.channels_last) or xn.shape[1] == 1 or xn.shape[2] * xn.shape[3] == 1
    y3, flat3 = F.max_pool2d(xn, c["k"], c["s"], c["p"], return_indices=True)
    y4, flat4 = F.max_pool2d(xn.contiguous(), c["k"], c["s"], c["p"], return_indices=True)
    assert _eq_nan(y3, y4) and torch.equal(flat3, flat4)


def test_pool_cases_reach_what_they_name():
    assert {(c["k"], c["s"], c["p"]) for c in R.POOL} == {(2, 2, 0), (3, 1, 1), (5, 1, 2), (3, 2, 1), (2, 1, 1), (4, 3, 2), (7, 2, 3), (15, 1, 7), (15, 15, 0)}
    assert {c["dtype"] for c in R.POOL} == {F16, F32}
    assert {c["C"] // R.NGRP[c["dtype"]] for c in R.POOL} >= {1, 2, 3}
    totals = {t for c in R.POOL for t in R.pool_threads(c)}
    assert 255 in totals and 257 in totals
    assert sum(R.pool_threads(c) == (255, 255) for c in R.POOL) == 1 and sum(R.pool_threads(c) == (257, 257) for c in R.POOL) == 1
    uncovered = []
    for c in R.POOL:
        Ho, Wo = R.pool_out(c["H"], c["k"], c["s"], c["p"]), R.pool_out(c["W"], c["k"], c["s"], c["p"])
        last_h, last_w = (Ho - 1) * c["s"] - c["p"] + c["k"] - 1, (Wo - 1) * c["s"] - c["p"] + c["k"] - 1
        if last_h < c["H"] - 1 or last_w < c["W"] - 1:
            uncovered.append((c["k"], c["s"], c["p"]))
            dx = R.pool_reference(c["name"])[2]
            assert float(dx[:, last_h + 1:].abs().max() if last_h < c["H"] - 1 else 0) == 0 and float(dx[:, :, last_w + 1:].abs().max() if last_w < c["W"] - 1 else 0) == 0
    assert set(uncovered) == {(2, 2, 0), (15, 15, 0)}                                  # (with padding >= (k - stride) / 2 no pixel is left out)
    assert any(c["H"] == 1 and c["W"] == 1 and (c["k"], c["p"]) == (3, 1) for c in R.POOL)
    assert sum(c["H"] + 2 * c["p"] == c["k"] for c in R.POOL) >= 3 and any(c["H"] + 2 * c["p"] == c["k"] and c["W"] + 2 * c["p"] == c["k"] for c in R.POOL)
    assert any(R.pool_out(c["H"], c["k"], c["s"], c["p"]) > c["H"] for c in R.POOL)
    special = [c for c in R.POOL if c["fill"] == "special"]
    assert len(special) == 3
    for c in special:
        x = R.pool_inputs(c["name"])["x"]
        y, idx, dx = R.pool_reference(c["name"])
        assert int((y == NEG).sum()) > 0 and int(torch.isnan(y).sum()) > 0 and int(((y != NEG) & ~torch.isnan(y)).sum()) > 0
        assert int(torch.isnan(y[..., -1]).sum()) < int(torch.isnan(y[..., 0]).sum())   # the pixel that is NaN in half of the channels
    for c in R.POOL:
        if c["fill"] == "ties":                                                        # tie-heavy: most windows hold their maximum more than once
            x = R.pool_inputs(c["name"])["x"]
            assert x.unique().numel() <= 3


def test_upsample_reference_and_cases():
    for c in R.UP:
        i = R.up_inputs(c["name"])
        y, dx = R.up_ref(i["x"], i["dy"])
        xn = i["x"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yn = F.interpolate(xn, scale_factor=2, mode="nearest")
        yn.backward(i["dy"].double().permute(0, 3, 1, 2))
        assert torch.equal(yn.detach().permute(0, 2, 3, 1), y.double()) and torch.equal(xn.grad.permute(0, 2, 3, 1), dx)
        assert torch.equal(dx.to(c["dtype"]).double(), dx)
    assert any(c["B"] % 2 and c["H"] % 2 and c["W"] % 2 and c["B"] > 1 for c in R.UP) and any(c["H"] == c["W"] == 1 for c in R.UP)
    tot = {c["B"] * c["H"] * c["W"] * c["C"] // R.NGRP[c["dtype"]] for c in R.UP}
    assert {255, 257} <= tot and {c["dtype"] for c in R.UP} == {F16, F32}


def test_join_reference_and_cases():
    assert float(R.ulp(torch.tensor(1.0).double(), F16)) == 2.0 ** -10 and float(R.ulp(torch.tensor(1.5).double(), F32)) == 2.0 ** -23
    assert float(R.ulp(torch.tensor(2.0 ** -20).double(), F16)) == 2.0 ** -24 and float(R.ulp(torch.tensor(0.0).double(), F16)) == 2.0 ** -24      # subnormals
    assert {len(c["levels"]) for c in R.JOIN} == {1, 2, 3, 4} and {c["levels"] for c in R.JOIN} >= {(1,), (5, 3, 1), (64, 16, 4, 1)}
    assert {c["nc"] for c in R.JOIN} == {4, 12, 80} and {c["nreg"] for c in R.JOIN} == {4, 68}
    assert any(R.pad_to(c["nreg"], c["dtype"]) == 72 and c["nreg"] == 68 for c in R.JOIN) and any(R.pad_to(c["nc"], c["dtype"]) == 16 and c["nc"] == 12 for c in R.JOIN)
    for c in R.JOIN:
        i, ref = R.join_inputs(c["name"]), R.join_reference(c["name"])
        for t in i["cls"]:
            v = t.double().view(-1)
            assert float(v.max()) == 12 and float(v.min()) == -12 and bool((v == 0).any()) if v.numel() >= 3 else True
        x = torch.cat([t.double() for t in i["cls"]], 1).requires_grad_(True)
        torch.sigmoid(x).backward(i["d_cls"].double())
        y64 = torch.sigmoid(x.detach())
        assert torch.equal(ref["cls"], y64)
        # the backward reads the STORED y: the reference is d (1 - y) y of that value, which differs from autograd's by the rounding of y alone
        assert float((x.grad - ref["dl"]).abs().max()) <= float((i["d_cls"].double().abs() * (y64 - i["y"].double()).abs()).max()) + 1e-12
        assert bool((ref["cls_bound"] > 0).all()) and bool((ref["dl_bound"] > 0).all())
        assert torch.equal(torch.cat(R.split_levels(ref["dreg"], c["levels"]), 1), i["d_reg"])


def test_sum_and_colsum_cases():
    assert {(c["n"], c["acc"], c["dtype"]) for c in R.SUM} == {(n, a, d) for n in (1, 2, 3, 4) for a in (0, 1) for d in (F16, F32)}
    for c in R.SUM:
        i = R.sum_inputs(c["name"])
        ref = R.sum_ref(i["src"], i["dst"], c["acc"])
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 15 and (c["M"] * c["C"] // R.NGRP[c["dtype"]]) % 256 != 0
    assert {c["C"] for c in R.COL} == set(R.COL_C) | {R.COL_CAP[0]}
    pers = [R.col_geom(1, C)["per"] for C in R.COL_C]
    assert pers == [256, 85, 3, 3, 3, 2, 2, 1, 1, 1]
    assert [R.col_geom(1, C)["idle"] for C in R.COL_C] == [0, 1, 52, 16, 1, 84, 0, 127, 1, 0]
    for C in R.COL_C:
        per = max(256 // C, 1)
        ms = sorted(c["M"] for c in R.COL if c["C"] == C and "cap" not in c["name"])
        assert set(ms) == {1, 7, 8 * per - 1, 8 * per, 8 * per + 1, 64 * per + 1}, (C, ms)
        for M in (8 * per - 1, 8 * per, 8 * per + 1):
            g = R.col_geom(M, C)
            assert g["nb"] == 1 and g["step"] == per                                   # one workgroup: 8 x the grid stride is 8 per
        assert R.col_geom(64 * per + 1, C)["nb"] == 2
    g = R.col_geom(R.COL_CAP[1], R.COL_CAP[0])
    assert g["want"] == 1025 and g["nb"] == 1024 and g["per"] == 1
    assert sum(R.col_geom(c["M"], c["C"])["want"] > 1024 for c in R.COL) == 1
    for c in R.COL:
        i = R.col_inputs(c["name"])
        assert float(i["x"].double().abs().sum(0).max()) + 9 < 2 ** 24 and float(i["pre"].abs().min()) > 0
    assert {c["dtype"] for c in R.COL} == {F16, F32}
