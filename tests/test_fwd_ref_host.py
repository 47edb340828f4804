"""The references and the checker of tests/test_gpu_fwd_edges.py, on the CPU: every fp64 reference of tests/fwd_ref.py against plain F.conv2d / F.max_pool2d /
F.interpolate in float64 on the very tensors the GPU test uses, the preconditions of family E, and — for every case and every mutation that exists in it — that the
reference of the mutated input differs from the true one by more than the checker allows (family E: at all; family B: by more than the bound)."""
import pytest
import torch
import torch.nn.functional as F

from maf_yolo_amd import conv_variants, lib, pack

import fwd_ref as R
import op_ref

ALL = [c["name"] for c in R.CASES]


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _act(y, act):
    return {lib.ACT_NONE: lambda v: v, lib.ACT_RELU: F.relu, lib.ACT_SILU: F.silu, lib.ACT_SIGMOID: torch.sigmoid}[act](y)


def _plain_src(x, mode, H, W):
    x = _nchw(x)
    if mode == lib.SRC_UP2:
        return F.interpolate(x, size=(H, W), mode="nearest")
    if mode == lib.SRC_POOL2:
        return F.max_pool2d(x, 2, 2)
    if mode == lib.SRC_SUB2:
        return F.conv2d(x, torch.eye(x.shape[1], dtype=torch.float64).reshape(x.shape[1], x.shape[1], 1, 1), stride=2)     # a 1x1 conv with stride 2
    return x


def _plain(c, inp):
    """{output: NHWC float64} of the case by torch's own operators."""
    kind = c["kind"]
    H, W = R.out_grid(c)
    out = {}
    if kind == "conv1":
        for key, o in (("out", inp), ("twin", inp.get("twin"))):
            if o is not None:
                x = torch.cat([_plain_src(s, m, H, W) for s, (_, m) in zip(o["srcs"], c["srcs"])], 1)
                out[key] = _act(F.conv2d(x, o["w"].double(), o["b"].double()), c["act"])
    elif kind == "conv3":
        for key, o in (("out", inp), ("twin", inp.get("twin"))):
            if o is not None:
                out[key] = _act(F.conv2d(_nchw(o["srcs"][0]), o["w"].double(), o["b"].double(), 2, 1), c["act"])
        if c.get("nc"):
            w1, b1 = inp["pool1"]
            out["pool"] = F.silu(F.conv2d(F.max_pool2d(_nchw(inp["srcs"][0]), 2, 2), w1.double(), b1.double()))
    elif kind == "dw":
        x = _nchw(inp["srcs"][0])
        if c["two"]:
            x = torch.cat([x, x], 1)
        out["out"] = _act(F.conv2d(x, inp["w"].double(), inp["b"].double(), 1, c["k"] // 2, 1, x.shape[1]), c["act"])
    elif kind == "fused":                                         # the fp16 rounding points of the kernels (and of test_gpu_kernels.py): T1, T2, y
        def r16(t):
            return t.half().double()
        raw, k, mid = inp["raw"], c["k"], 3 * c["c"]
        t = r16(F.silu(F.conv2d(_nchw(inp["srcs"][0]), raw[0].double(), raw[1].double())))
        y = F.silu(F.conv2d(t, inp["w"].double(), raw[3].double(), 1, k // 2, 1, mid))
        if c["sub"] != "c1dw":
            y = F.silu(F.conv2d(r16(y), raw[4].double(), raw[5].double()))
        if c["sub"] == "tail":
            y = F.silu(F.conv2d(torch.cat([_nchw(s_) for s_ in inp["srcs"][1:]] + [_nchw(inp["srcs"][0]), r16(y)], 1), raw[6].double(), raw[7].double()))
        out["out"] = y
    elif kind == "head":                                          # test_gpu_fused_parity.py's restatement, in float64
        from oracle import maf_oracle as O
        raw, B = inp["raw"], c["B"]
        t = [F.silu(F.conv2d(_nchw(inp["srcs"][i]), raw[4 * i].double(), raw[4 * i + 1].double())).half().double() for i in range(2)]
        cls = torch.sigmoid(F.conv2d(t[0], raw[2].double(), raw[3].double()))
        reg = F.conv2d(t[1], raw[6].double(), raw[7].double())
        return {"out": O.decode([(torch.zeros(B, 1, H, W, dtype=torch.float64), cls, reg)], strides=(float(c["stride"]),))}
    elif kind == "stem2":                                         # the image and the half-resolution tensor are fp16 in the kernel
        x = inp["image"].float()
        x = (x * torch.tensor(1.0 / 255.0)).half() if c["in_dtype"] == "u8" else x.half()
        raw = inp["raw"]
        t = F.relu(F.conv2d(x.double(), inp["w"].double(), raw[1].double(), 2, 1)).half().double()
        y = F.relu(F.conv2d(t, raw[2].double(), raw[3].double(), 2, 1))
        if c["third"]:
            y = F.silu(F.conv2d(y.half().double(), raw[4].double(), raw[5].double()))
        h = c["cout"] // 2
        out.update({"out": y[:, :h], "out2": y[:, h:]} if c["split"] else {"out": y})
    elif kind == "stem":
        x = inp["image"].float()
        if c["in_dtype"] == "u8":
            x = x * torch.tensor(1.0 / 255.0)
        out["out"] = F.relu(F.conv2d(x.double(), inp["w"].double(), inp["b"].double(), 2, 1))
    else:
        x = _nchw(inp["srcs"][0])
        ys = []
        for _ in range(3):
            x = F.max_pool2d(x, 5, 1, 2)
            ys.append(x)
        out["out"] = torch.cat(ys, 1)
    return {k: v.permute(0, 2, 3, 1) for k, v in out.items()}


@pytest.mark.parametrize("name", ALL)
def test_reference_is_torchs_own_operator_in_float64(name):
    c = R.BY_NAME[name]
    ref = R.case_reference(c)
    plain = _plain(c, R.inputs(c))
    assert set(ref) == set(plain)
    for k, (r, bnd, _) in ref.items():
        assert r.dtype == torch.float64 and r.shape == plain[k].shape
        if R.is_exact(c, k):
            assert torch.equal(r, plain[k]), (name, k)
        else:
            assert bool(((r - plain[k].to(r.dtype)).abs() <= (1e-12 if plain[k].dtype == torch.float64 else 1e-5) * (1 + r.abs())).all()), (name, k)        # fp64 summation order: thirteen digits, four under the tightest bound
        assert bool((bnd > 0).all())


@pytest.mark.parametrize("name", [n for n in ALL if R.BY_NAME[n]["family"] == "E" and R.BY_NAME[n]["kind"] != "sppf"])
def test_family_e_is_exact_in_fp32_and_in_the_store(name):
    c = R.BY_NAME[name]
    inp, ref = R.inputs(c), R.case_reference(c)
    assert c["act"] in (lib.ACT_NONE, lib.ACT_RELU)
    for o in (inp, inp.get("twin")):
        if o is None:
            continue
        ts = list(o["srcs"]) + ([o["w"], o["b"]] if "b" in o else o["raw"]) + ([o["image"]] if "image" in o else [])
        amp = max(float(t.abs().max()) for t in ts)
        assert all(torch.equal(t.double(), t.double().round()) for t in ts) and amp <= R.AMP
        assert (R.n_terms(c) + 1) * amp * amp < 2 ** 22
        if c["kind"] == "stem2":                                 # the second stage: 9 C0 products of an fp16 integer <= 27 + 1 of the first
            assert amp == 1 and (9 * c["C0"] + 1) * 28 < 2 ** 22
    for k, (r, _, _) in ref.items():
        if k == "pool":
            continue                                             # (the pooled branch's SiLU is hard-wired: that output is checked against the bound)
        assert torch.equal(r, r.round())
        if R.store_dtype(c) == torch.float16:
            assert float(r.abs().max()) <= 2048
        assert torch.equal(r.to(R.store_dtype(c)).double(), r)


@pytest.mark.parametrize("name", ALL)
def test_every_mutation_moves_the_reference_past_the_checker(name):
    c = R.BY_NAME[name]
    ref = R.case_reference(c)
    assert c["muts"]
    for mut in c["muts"]:
        bad = R.reference(c, mut=mut)
        moved = False
        for k, (r, bnd, _) in ref.items():
            d = (bad[k][0] - r).abs()
            d = torch.where(torch.isnan(d), torch.zeros_like(d), d)         # (-inf against -inf in SPPF's poisoned channel)
            if R.is_exact(c, k):
                moved |= bool((d > 0).any()) and not torch.equal(bad[k][0].to(R.store_dtype(c)), r.to(R.store_dtype(c)))
            else:
                moved |= bool((d > bnd).any())
        assert moved, "%s: mutation %s stays inside the checker" % (name, mut)


def test_the_mutations_named_all_exist_somewhere():
    seen = {m for c in R.CASES for m in c["muts"]}
    assert seen == set(R.MUTATIONS)
    for kind, need in (("conv1", {"kstep", "row", "col", "batch", "up2", "pool2", "chunk"}), ("conv3", {"tap", "kstep", "row", "col", "batch", "chunk"}),
                       ("dw", {"tap", "kstep", "row", "col", "batch", "chunk"}), ("stem", {"tap", "row", "col", "batch", "div255"}), ("sppf", {"row", "col", "batch", "kstep", "chunk"}), ("fused", {"tap", "row", "col", "batch", "kstep", "chunk"}), ("stem2", {"tap", "row", "col", "batch", "div255"}), ("head", {"row", "col", "batch", "kstep", "chunk"})):
        assert need <= {m for c in R.CASES if c["kind"] == kind for m in c["muts"]}, kind


def _tiles(c):
    """What tests/test_gpu_fwd_edges.py asks conv_variants.conv_tiles for (any output stride that is a multiple of 8)."""
    kind = lib.OP_CONV3X3S2 if c["kind"] == "conv3" else lib.OP_CONV1X1
    H, W = R.out_grid(c)
    dt = lib.F16 if c["dtype"] == "f16" else lib.F32
    out = []
    for M in (c["B"] * H * W, 65536):
        out += conv_variants.conv_tiles(kind, dt, M, c["srcs"], c["cout"], 8, bool(c.get("out_f32")), bool(c.get("twin")))
    out += c.get("extra", [])
    return [t for t in dict.fromkeys(out) if not c.get("only") or t[2] in c["only"]]


def test_the_cases_reach_every_variant_the_issue_names():
    """By shape alone: the lists of conv_variants.conv_tiles for the cases (plus the explicit tiles a case names) hold every variant family, the DMA ring on
    (tile_p, tile_c) in {1, 2} x {4, 6, 8} for all three VARs, split-K at 8 .. 11 steps and CONV_STREAM_LDS at both ends of its step ranges."""
    fams = {}
    for c in R.CASES:
        if c["kind"] in ("conv1", "conv3"):
            for t in _tiles(c):
                fams.setdefault((c["kind"], t[2]), []).append((c, t))
    for tk in (lib.CONV_GENERIC, lib.CONV_LDS, lib.CONV_DMA, lib.CONV_SPLITK, lib.CONV_STREAM, lib.CONV_STREAM_LDS):
        assert ("conv1", tk) in fams, tk
    for tk in (lib.CONV_GENERIC, lib.CONV_LDS, lib.CONV_DMA, lib.CONV_SPLITK, lib.CONV3_LDS, lib.CONV3_WREG):
        assert ("conv3", tk) in fams, tk
    assert {t[0] for _, t in fams[("conv1", lib.CONV_STREAM_LDS)]} == {1, 2} and {t[0] for _, t in fams[("conv1", lib.CONV_STREAM)]} == {1, 2}

    def steps(c):
        return sum(-(-s[0] // 32) for s in c["srcs"]) * (9 if c["kind"] == "conv3" else 1)
    ring = {(pt, ct) for pt in (1, 2) for ct in (4, 6, 8)}
    for var, pred in (("direct", lambda c: c["kind"] == "conv1" and len(c["srcs"]) == 1), ("multi", lambda c: c["kind"] == "conv1" and len(c["srcs"]) > 1), ("3x3", lambda c: c["kind"] == "conv3")):
        dma = [(c, t) for k in ("conv1", "conv3") for c, t in fams[(k, lib.CONV_DMA)] if pred(c)]
        assert {t[:2] for _, t in dma} >= ring, var
        st = {steps(c) for c, _ in dma}
        assert any(s % 2 for s in st) and {-(-s // 2) % 4 for s in st} >= {1, 2, 3} and (var == "3x3" or any(-(-s // 2) < 4 for s in st)), (var, st)      # (nine taps: never fewer than 5 stages)
    assert {steps(c) for c, _ in fams[("conv1", lib.CONV_SPLITK)]} >= {8, 9, 10, 11}
    assert {steps(c) for c, _ in fams[("conv1", lib.CONV_STREAM_LDS)]} >= {2, 12, 13, 20, 24, 26}
    assert {(c["srcs"][0][0], c["cout"]) for c, _ in fams[("conv3", lib.CONV3_WREG)]} == {s for s in R.WREG_SHAPES if pack.conv3x3_wreg_shape(*s)} == set(R.WREG_SHAPES)
    assert {(c["srcs"][0][0], c["cout"]) for c, _ in fams[("conv3", lib.CONV3_LDS)]} == {(48, 48), (48, 64), (64, 64)}
    for tk in (lib.CONV_GENERIC, lib.CONV_LDS, lib.CONV_DMA, lib.CONV_SPLITK):
        assert any(c.get("twin") for k in ("conv1", "conv3") for c, _ in fams[(k, tk)] if c["kind"] == k), tk


def test_every_case_names_its_branch():
    for c in R.CASES:
        assert len(c["why"]) > 10, c["name"]
    ms = {c["B"] * c["H"] * c["W"] for c in R.CASES if c["kind"] == "conv1"}
    assert ms >= {15, 16, 17, 63, 65, 129}
    assert sum(1 for m in (15, 16, 17, 63, 65, 129) if R.M_BHW[m][0] > 1) >= 2


def test_ulp_and_bound_are_op_refs():
    x = torch.tensor([1.0, 1000.0, 1e-9], dtype=torch.float64)
    assert torch.equal(op_ref.ulp(x), torch.tensor([2.0 ** -10, 0.5, 2.0 ** -24], dtype=torch.float64))
    assert (op_ref.K_CONV, op_ref.R16, op_ref.K_STAGE) == (2, 2, 0.25)
