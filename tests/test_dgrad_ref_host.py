"""The data-gradient references of tests/test_gpu_dgrad_edges.py (tests/dgrad_ref.py) checked on the CPU: against torch.autograd of F.conv2d in float64, and — for
EVERY case of the table, on the very tensors the GPU test uses — what the exact comparison rests on: the headroom rule of int_case, every element of the reference
(and of each addend of the RepVGG pair) an integer of magnitude <= 2048 (fp16 stores it exactly, a change of 1 is visible), and that each mutation a wrong kernel
could amount to — a dropped tap, an unflipped filter, swapped parities, an ignored last row or column of dY, swapped images, a channel chunk read from chunk 0 —
changes the case's reference."""
import pytest
import torch
import torch.nn.functional as F

from maf_yolo_amd import lib, train_ops

import dgrad_ref as D
from dgrad_ref import conv_dgrad_ref, dw_branches_dgrad_ref, dw_dgrad_ref, repvgg_dgrad_ref
from wgrad_ref import int_case, wide_case


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _autograd(dy, w, s, H, W, groups=1):
    """d/dx of sum(conv2d(x, w) * dy) in float64: dy NHWC, w in conv2d's layout; NHWC result."""
    k = w.shape[-1]
    x = torch.zeros(dy.shape[0], w.shape[1] * groups, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, s, k // 2, 1, groups).backward(dy.double().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1)


def _close(got, want, S):
    return float((got - want).abs().max()) <= 1e-12 * max(float(S.max()), 1e-300)


# B, H, W, Cin, Cout, k, s
CONV_SHAPES = [(2, 6, 8, 3, 4, 3, 2),       # even sides: the split form's geometry
               (2, 7, 5, 2, 3, 3, 2),       # odd sides
               (2, 5, 8, 3, 2, 3, 2),       # odd H, even W
               (3, 1, 6, 2, 2, 3, 2),       # H = 1: only the centre tap row lands inside
               (1, 1, 1, 1, 1, 3, 2),       # one pixel
               (2, 2, 2, 2, 3, 3, 2),       # H < k
               (2, 6, 4, 3, 2, 1, 2),       # k = 1 s = 2, even sides: the odd pixels get nothing
               (2, 7, 5, 3, 2, 1, 2),       # k = 1 s = 2, odd sides
               (2, 5, 4, 3, 5, 1, 1)]


@pytest.mark.parametrize("B,H,W,cin,cout,k,s", CONV_SHAPES)
def test_conv_reference_matches_autograd_of_conv2d_in_float64(B, H, W, cin, cout, k, s):
    g = _gen(H * 10 + W + k)
    dy, w = wide_case((B, _out(H, k, s), _out(W, k, s), cout), g), wide_case((cout, cin, k, k), g)
    got, S, n = conv_dgrad_ref(dy, w, k, s, H, W)
    assert got.dtype == torch.float64 and got.shape == (B, H, W, cin)
    want, wantS = _autograd(dy, w, s, H, W), _autograd(dy.abs(), w.abs(), s, H, W)
    assert _close(got, want, wantS) and _close(S, wantS, wantS) and bool((S >= got.abs()).all())
    assert n == int(_autograd(torch.ones_like(dy), torch.ones_like(w), s, H, W).max())          # products per element: counted by a conv of ones
    di, wi = int_case(dy.shape, g), int_case(w.shape, g)
    goti, Si, ni = conv_dgrad_ref(di, wi, k, s, H, W, exact=True)
    assert goti.dtype == torch.int64 and ni == n and torch.equal(goti.double(), _autograd(di, wi, s, H, W)) and torch.equal(Si.double(), _autograd(di.abs(), wi.abs(), s, H, W))


@pytest.mark.parametrize("B,H,W,C,k", [(2, 5, 4, 3, 3), (2, 7, 5, 2, 5), (1, 2, 9, 2, 9), (3, 5, 1, 2, 7), (2, 4, 6, 3, 1), (1, 1, 1, 1, 9), (2, 2, 3, 8, 7)])
def test_depthwise_reference_matches_autograd_of_conv2d_in_float64(B, H, W, C, k):
    g = _gen(H * 10 + W + k)
    dy, w = wide_case((B, H, W, C), g), wide_case((C, 1, k, k), g)
    got, S, n = dw_dgrad_ref(dy, w, k)
    want, wantS = _autograd(dy, w, 1, H, W, C), _autograd(dy.abs(), w.abs(), 1, H, W, C)
    assert _close(got, want, wantS) and _close(S, wantS, wantS)
    assert n == int(_autograd(torch.ones_like(dy), torch.ones_like(w), 1, H, W, C).max())
    di, wi = int_case(dy.shape, g), int_case(w.shape, g)
    goti, _, _ = dw_dgrad_ref(di, wi, k, exact=True)
    assert goti.dtype == torch.int64 and torch.equal(goti.double(), _autograd(di, wi, 1, H, W, C))


@pytest.mark.parametrize("k0", [3, 5, 7, 9])
@pytest.mark.parametrize("H,W", [(6, 10), (3, 5)])
def test_branch_sum_reference_matches_autograd_of_the_summed_convs(k0, H, W):
    g = _gen(k0 + H)
    ks = D.DWB_SETS[k0]
    dys, ws = [int_case((2, H, W, 3), g) for _ in ks], [int_case((3, 1, k, k), g) for k in ks]
    got, S, n = dw_branches_dgrad_ref(dys, ws, exact=True)
    want = sum(_autograd(dy, w, 1, H, W, 3) for dy, w in zip(dys, ws))
    assert torch.equal(got.double(), want) and n == sum(int(_autograd(torch.ones_like(dy), torch.ones_like(w), 1, H, W, 3).max()) for dy, w in zip(dys, ws))
    assert torch.equal(S.double(), sum(_autograd(dy.abs(), w.abs(), 1, H, W, 3) for dy, w in zip(dys, ws)))


@pytest.mark.parametrize("H,W", [(8, 16), (4, 8), (2, 2)])
def test_repvgg_reference_matches_autograd_of_the_two_convs(H, W):
    g = _gen(H)
    dz3, dz1 = int_case((2, H // 2, W // 2, 5), g), int_case((2, H // 2, W // 2, 5), g)
    w3, w1 = int_case((5, 3, 3, 3), g), int_case((5, 3, 1, 1), g)
    dx, S, n, a3, a1 = repvgg_dgrad_ref(dz3, dz1, w3, w1, H, W, exact=True)
    x = torch.zeros(2, 3, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w3.double(), None, 2, 1) * dz3.double().permute(0, 3, 1, 2)).sum().backward()
    g3 = x.grad.clone()
    (F.conv2d(x, w1.double(), None, 2, 0) * dz1.double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(dx.double(), x.grad.permute(0, 2, 3, 1)) and torch.equal(a3[0].double(), g3.permute(0, 2, 3, 1)) and torch.equal(a3[0] + a1[0], dx)
    assert (n, a3[2], a1[2]) == ((2 * 5, 5, 5) if H == 2 else (4 * 5, 4 * 5, 5)) and torch.equal(S, a3[1] + a1[1])     # the 1x1 lands where ONE 3x3 tap does
    assert int(a1[0][:, 1::2].abs().max()) == 0 and int(a1[0][:, :, 1::2].abs().max()) == 0           # the 1x1 branch lives on the even pixels


# ------------------------------------------------------------------------------------------------------------------- every case of the table, on its own tensors
def test_the_1x1_cases_reach_every_form_the_training_tuner_offers_on_a_transposed_pack():
    """(tile_p, variant) over the candidate lists of all 1x1 cases: besides tile_p 1 of every variant and the two-tile stream forms, the generic kernel at tile_p 2 and
    4 and the LDS-shared-weight kernel at tile_p 2 — offered only where pixels x channel tiles fill the chip (M 4551 into 576 channels)."""
    forms = set()
    for c in D.CASES:
        if c["kind"] == "conv1" and c["dtype"] == "f16" and "autograd" not in c["name"]:
            forms |= {(pt, tk) for pt, _, tk in train_ops.conv_candidates(c["B"] * c["H"] * c["W"], -(-c["cout"] // 8) * 8, c["cin"])}
    assert forms >= {(1, lib.CONV_GENERIC), (2, lib.CONV_GENERIC), (4, lib.CONV_GENERIC), (1, lib.CONV_LDS), (2, lib.CONV_LDS), (1, lib.CONV_SPLITK), (1, lib.CONV_DMA),
                     (1, lib.CONV_STREAM), (2, lib.CONV_STREAM), (1, lib.CONV_STREAM_LDS), (2, lib.CONV_STREAM_LDS)}, sorted(forms)


ALL = [c["name"] for c in D.CASES]
EXACT = [c["name"] for c in D.CASES if c["family"] == "E"]


def test_the_table_covers_what_the_gpu_file_promises():
    c3 = [c for c in D.CASES if c["kind"] == "conv3" and c["family"] == "E" and c["dtype"] == "f16"]
    split = sorted(c["B"] * (c["H"] // 2) * (c["W"] // 2) for c in c3 if c["H"] % 2 == 0 and c["W"] % 2 == 0 and c["name"].startswith("conv3-split"))
    assert split == [1, 63, 64, 65, 127, 129, 576]
    assert {(c["H"], c["W"]) for c in c3 if c["H"] % 2 or c["W"] % 2} >= {(5, 8), (8, 5), (5, 7), (1, 1), (1, 6), (3, 2)}
    assert {c["cout"] for c in c3} >= {8, 24, 48, 72, 200, 32, 128, 384} and {c["cin"] for c in c3} >= {8, 24, 40, 200, 128} and all(c["B"] >= 2 for c in c3 if "split" not in c["name"])
    c1 = [c for c in D.CASES if c["kind"] == "conv1" and c["family"] == "E" and c["dtype"] == "f16" and "autograd" not in c["name"]]
    assert {(c["cout"], c["cin"]) for c in c1} == set(D.CONV1_SHAPES) and {c["B"] * c["H"] * c["W"] for c in c1} == {15, 16, 17, 63, 65, 4551}
    for co, ci in D.CONV1_SHAPES:
        assert {c["B"] * c["H"] * c["W"] for c in c1 if (c["cout"], c["cin"]) == (co, ci)} == {15, 16, 17, 63, 65, 4551}
    dw = [c for c in D.CASES if c["kind"] == "dw" and c["family"] == "E" and c["dtype"] == "f16"]
    for k in (3, 5, 7, 9):
        assert {(c["H"], c["W"]) for c in dw if c["k"] == k} == {(2, 3), (4, 4), (9, 13), (20, 20), (33, 7)} and {c["C"] for c in dw if c["k"] == k} == {8, 24, 72, 200}
    dwb = [c for c in D.CASES if c["kind"] == "dwb" and c["family"] == "E" and c["dtype"] == "f16" and "unused" not in c]
    assert {(c["k0"], c["H"], c["W"]) for c in dwb} == {(k0, h, w) for k0 in (3, 5, 7, 9) for h, w in ((6, 10), (20, 24), (3, 5))}
    rv = [c for c in D.CASES if c["kind"] == "repvgg" and c["family"] == "E"]
    assert {(c["cin"], c["cout"], c["B"], c["H"], c["W"]) for c in rv} == {(ci, co, b, h, w) for ci, co in ((24, 48), (8, 24), (96, 96)) for b, h, w in ((2, 8, 16), (1, 4, 8))}
    assert all(c["why"] and set(c["muts"]) <= set(D.MUTATIONS) for c in D.CASES)


@pytest.mark.parametrize("name", EXACT)
def test_exact_case_keeps_the_headroom_and_fits_fp16_exactly(name):
    c = D.BY_NAME[name]
    inp = D.inputs(c)
    for t in inp["dys"] + inp["ws"]:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
    dx, S, n, parts = D.case_reference(c)
    assert dx.dtype == torch.int64 and n * 3 * 3 < 2 ** 22                 # int_case's rule: two bits under 2^24 whatever the order of the adds
    assert int(S.max()) < 2 ** 22
    assert int(dx.abs().max()) <= 2048, "%s: |ref| reaches %d: change the seed" % (name, int(dx.abs().max()))
    if parts is not None:
        for a in parts:
            assert int(a[0].abs().max()) <= 2048 and a[2] * 9 < 2 ** 22
    if c.get("cin_w", c.get("cin")) != c.get("cin"):
        assert int(dx[..., c["cin_w"]:].abs().max()) == 0 and int(dx[..., :c["cin_w"]].abs().max()) > 0


@pytest.mark.parametrize("name", [c["name"] for c in D.CASES if c["family"] == "B"])
def test_bound_case_stays_inside_the_term_count_and_fp16_range(name):
    c = D.BY_NAME[name]
    dx, S, n, parts = D.case_reference(c)
    assert dx.dtype == torch.float64 and n <= 4096 and float(S.max()) < 60000 and bool((S >= dx.abs()).all())
    inp = D.inputs(c)
    a = torch.cat([t.reshape(-1).float().abs() for t in inp["dys"]])
    assert float(a.max()) > 64 and float(a[a > 0].min()) < 2.0 ** -8             # binades apart


def _taps_of(c):
    """[(drop, mask or None)]: every tap worth dropping in the case and, for the 3x3 stride-2 gradient, the parity class (rows, columns) it serves."""
    kind = c["kind"]
    if kind == "conv1" or kind == "conv1s2":
        return [((0, 0, 0), None)]
    if kind in ("conv3", "repvgg"):
        taps = [((0, ky, kx), ((ky + 1) % 2, (kx + 1) % 2)) for ky in range(3) for kx in range(3)]
        return taps + ([((1, 0, 0), (0, 0))] if kind == "repvgg" else [])
    ks = (c["k"],) if kind == "dw" else D.DWB_SETS[c["k0"]]
    out = []
    for j, k in enumerate(ks):
        if c.get("unused") == j:
            continue
        out += [((j, ky, kx), None) for ky, kx in {(0, 0), (0, k - 1), (k - 1, 0), (k - 1, k - 1), (k // 2, k // 2), (k // 2, 0), (0, k // 2)}]
    return out


def _serves(c, drop):
    """Whether the tap lands on a pixel of the map at all (3 x 3 stride 2 on a one-row map: only the centre row does; a 9 x 9 filter on a 2 x 3 map: the taps near
    its centre)."""
    H, W = c["H"], c["W"]
    if c["kind"] in ("conv3", "repvgg") and drop[0] == 0:
        ok = lambda n, t: any(0 <= 2 * o - 1 + t < n for o in range(n // 2 + n % 2))
        return ok(H, drop[1]) and ok(W, drop[2])
    if c["kind"] in ("dw", "dwb"):
        k = c["k"] if c["kind"] == "dw" else D.DWB_SETS[c["k0"]][drop[0]]
        return abs(drop[1] - k // 2) < H and abs(drop[2] - k // 2) < W
    return True


@pytest.mark.parametrize("name", ALL)
def test_every_mutation_that_exists_in_the_case_changes_its_reference(name):
    c = D.BY_NAME[name]
    ref = D.case_reference(c)
    muts = c["muts"]
    assert "tap" in muts and "row" in muts and "col" in muts
    served = 0
    for drop, cls in _taps_of(c):
        if not _serves(c, drop):
            assert torch.equal(D.reference(c, drop=drop)[0], ref[0]), (name, drop)          # a tap that never lands inside the map: nothing to tell
            continue
        served += 1
        d = D.reference(c, drop=drop)[0] != ref[0]
        assert bool(d.any()), "%s: dropping tap %s changes nothing" % (name, (drop,))
        if cls is not None:                                                                  # the change stays inside the parity class the tap serves
            inside = torch.zeros_like(d)
            inside[:, cls[0]::2, cls[1]::2] = True
            assert not bool((d & ~inside).any()), (name, drop)
    assert served >= 1
    if c["kind"] in ("conv3", "repvgg") and c["H"] % 2 == 0 and c["W"] % 2 == 0 and min(c["H"], c["W"]) >= 4:
        assert served >= 9                                                                   # split form: all four classes, 1 + 2 + 2 + 4 taps (a 2-pixel side has no dY row for tap 0)
    if "noflip" in muts:
        assert bool((D.reference(c, noflip=True)[0] != ref[0]).any()), name
    if "parity" in muts:
        for p in {"conv3": ("taps",), "conv1s2": ("sub2",), "repvgg": ("taps", "sub2")}[c["kind"]]:
            assert bool((D.reference(c, parity=p)[0] != ref[0]).any()), (name, p)
    for what in ("row", "col", "batch", "chunk"):
        if what in muts:
            assert bool((D.reference(c, D.mutate_inputs(D.inputs(c), what))[0] != ref[0]).any()), "%s: %s changes nothing" % (name, what)
    assert ("batch" in muts) == (c["B"] >= 2) and ("chunk" in muts) == (c.get("cout", c.get("C")) >= 16)
    assert ("noflip" in muts) == (c["kind"] in ("dw", "dwb"))
