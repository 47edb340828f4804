"""Host-side checks of tests/loss_ref.py (no GPU): the fp64 restatement reproduces the reference's own ComputeLoss (the fixtures of tools/make_golden_loss.py),
the conditions its bounds rest on hold for every case tests/test_gpu_loss_edges.py uses, and its per-element checks reject subtly wrong results.
Run with -s to see r32, K, the near-tie shares and the rejected mutations."""
import math

import numpy as np
import pytest
import torch

import loss_ref as R


def _fixture_case(g, ci, atss, nc):
    size = int(g["c%d_size" % ci])
    hw = [(size // s, size // s) for s in (8, 16, 32)]
    pts, st = R.anchors(hw, (8, 16, 32))
    scores, distri, targets = (torch.from_numpy(g["c%d_%s" % (ci, k)]) for k in ("scores", "distri", "targets"))
    B = scores.shape[0]
    gts, offs = R.host_gts(targets, B, size)
    boxes = R.decode_f32(distri, pts, st)
    if atss:
        gt, norm, info = R.atss_ref(R.anchor_boxes(pts, st), [h * w for h, w in hw], boxes, gts, offs, 9)
    else:
        gt, norm, info = R.tal_ref(scores, boxes, pts, gts, offs, nc)
    return R.terms_ref(scores, distri, pts, st, gts, gt, norm), info


@pytest.mark.parametrize("fixture,ci,atss", [("loss_cases", ci, a) for ci, a in ((0, False), (1, False), (3, False), (1, True), (3, True))] +
                         [("loss_cases_nc", ci, a) for ci in range(4) for a in (False, True)])
def test_fp64_restatement_reproduces_the_reference_fixtures(golden, fixture, ci, atss):
    """tal_ref / atss_ref + terms_ref on the fixture's inputs == the reference's ComputeLoss: loss and items to 5e-5, every gradient element to the fixture's
    own fp32 (ATSS score gradients: fp16, as stored) rounding under the per-element bound of loss_ref.  This ties the fp64 restatement to the reference
    itself, at nc = 80 (old fixture) and nc = 1, 3, 20 with a crowded image of duplicated and nested boxes (new fixture)."""
    g = golden(fixture)
    nc = int(g["c%d_nc" % ci]) if fixture == "loss_cases_nc" else 80
    res, info = _fixture_case(g, ci, atss, nc)
    n, near = R.near_share(info)
    assert near == 0, "the fixture case has a near-tied decision: compare it by hand"
    p = "a%d_" % ci if atss else "c%d_" % ci
    want = float(g[p + "loss"])
    out = res["out"]
    assert abs(out[0].item() - want) <= 5e-5 * abs(want)
    assert np.allclose(out[1:4].numpy(), g[p + "items"], rtol=5e-5, atol=0)
    gs = torch.from_numpy(g[p + "gscores"].astype(np.float64)); gd = torch.from_numpy(g[p + "gdistri"].astype(np.float64)).reshape(res["gd"].shape)
    # the fixture's gradients come from the reference's own fp32 assignment: its normalised metric and target-score sum are within 2^-16 relative of the
    # fp64 ones (loss_ref), and every gradient term is linear in the one, inverse in the other: 3 x 2^-16 S on top of K 2^-24 S
    k = R.K + 3 * 2 ** 8
    rs = R.grad_ratio(gs, res["gs"], res["Ss"], torch.float16 if g[p + "gscores"].dtype == np.float16 else torch.float32, k).max().item()
    rd, bad_bg, kinks = R.distri_ratio(gd, res, torch.float32, k)
    assert bad_bg == 0 and kinks == 0
    print("%s %s%d: worst gradient ratio scores %.3f distri %.3f (boxes %d)" % (fixture, "a" if atss else "c", ci, rs, rd, n))
    assert rs <= 1 and rd <= 1


@pytest.fixture(scope="module")
def assigned():
    """the fp64 assignment of every assigner case on the fp32 stand-ins of the device preprocessing and decode"""
    out = {}
    for name in R.ASSIGN_NAMES:
        c = R.assign_case(name)
        gts, offs, boxes = R.host_inputs(c)
        out[name] = (c, gts, offs, boxes) + R.assign_ref(c, gts, offs, boxes)
    return out


def test_near_tie_share_and_thresholds_of_every_gpu_case(assigned):
    """The cap of loss_ref (a condition, not a measurement): near-tied decisions involve at most 2 % of a case's boxes, none below 50 boxes — computed from
    the fp64 reference alone.  The crowded 640 x 640 case really exceeds kGtL boxes and kMulti multiply-claimed anchors in image 0, the T = 1500 case really
    drops its 60 rows with image ids outside the batch."""
    for name, (c, gts, offs, boxes, gt, norm, info) in assigned.items():
        n, near = R.near_share(info)
        print("%-18s boxes %4d near-tied %d (%.2f %%), foreground %d, multiply-claimed %s" % (name, n, near, 100.0 * near / max(n, 1), int((gt >= 0).sum()),
                                                                                                 [i["n_multi"] for i in info]))
        assert near <= R.NEAR_CAP * n and (n >= 50 or near == 0), name
    for name in R.ZERO_FILL:                                                      # the zero-metric fill is reached through scores that are exactly 0
        i0 = assigned[name][6][0]
        print("%-18s zero-metric picks that lie inside their box: %d, of them with a score of exactly 0: %d" % (name, i0["zero_inside"], i0["zero_score_inside"]))
        assert i0["zero_score_inside"] > 0, name
    info = assigned["tal_640_crowd"][6]
    assert info[0]["n"] > R.K_GTL and info[0]["n_multi"] > R.K_MULTI and info[1]["n"] == 3
    gt = assigned["tal_640_crowd"][4]
    assert int(gt[0].max()) < 600, "duplicates resolve to the first row"
    c = assigned["tal_T1500"][0]
    assert c["targets"].shape[0] == 1500 and int(assigned["tal_T1500"][2][-1]) == 1440


def test_plain_fp32_label_preprocessing_is_within_one_ulp_on_every_case():
    """check_targets asks the device preprocessing for one fp32 ulp of the image size against targets_ref; the reference's own fp32 sequence (three
    roundings) can be 1.25 ulp off.  The cases are chosen so that it is within one: a condition of the cases, computed here without any kernel."""
    worst = 0.0
    todo = [(c["targets"], c["B"], c["size"]) for c in map(R.assign_case, R.ASSIGN_NAMES)]
    todo += [(R.terms_case(nc, dt, size, B)["targets"], B, size) for nc, dt, size, B in R.terms_cases()] + [(R.background_case(torch.float32)["targets"], 3, 64)]
    for t, B, size in todo:
        g, _ = R.host_gts(t, B, size)
        rows = R.targets_ref(t, B, size)[0]
        worst = max(worst, float((g.double()[:, 1:] - rows[:, 1:]).abs().max() / R.ulp(torch.tensor(float(size)), torch.float32)))
    print("fp32 label preprocessing against fp64: worst %.3f ulp of the image size" % worst)
    assert worst <= 1


def test_decode_r32_is_below_a_quarter_of_k_dec(assigned):
    """K_DEC of loss_ref, the bound of loss_decode_kernel, is 4 x the error of torch's fp32 softmax-expectation decode against decode_ref in units of
    2^-24 S over every assigner case (fp16 logits upcast exactly), rounded up to a power of two."""
    r32 = 0.0
    for name, (c, gts, offs, boxes, gt, norm, info) in assigned.items():
        ref, S = R.decode_ref(c["distri"], c["points"], c["stride"])
        r32 = max(r32, float(((boxes.double() - ref).abs() / (2.0 ** -24 * S)).max()))
    print("decode r32 = %.2f, K_DEC = %d" % (r32, R.K_DEC))
    assert r32 < R.K_DEC / 4 and R.K_DEC == 2 ** math.ceil(math.log2(4 * r32))
    assert {assigned[n][0]["distri"].dtype for n in R.F16_DISTRI} == {torch.float16}


@pytest.mark.parametrize("atss", [False, True])
def test_fp64_restatement_on_the_empty_batch_fixture(golden, atss):
    """Case c2 of the nc = 80 fixture has no labels: the reference divides the classification sum by a zero target-score sum (inf) and its box loss returns
    zeros; terms_ref's all-background path gives the same items."""
    g = golden("loss_cases")
    assert g["c2_targets"].shape[0] == 0
    res, info = _fixture_case(g, 2, atss, 80)
    p = "a2_" if atss else "c2_"
    out = res["out"]
    assert float(out[0]) == float(g[p + "loss"]) == math.inf and np.array_equal(out[1:4].numpy(), g[p + "items"].astype(np.float64))
    assert float(out[1]) == 0 and float(out[2]) == 0 and float(out[4]) == 0 and float(res["gd"].abs().max()) == 0


def test_fp32_oracle_against_fp64_metric(assigned):
    """oracle.maf_oracle (fp32, per box, torch.topk) against this module on every case it can run (3 square levels for ATSS; any for TAL): the worst difference of the normalised metric as a share of its maximum (recorded in loss_ref)."""
    from oracle import maf_oracle as O
    worst, differ = {False: 0.0, True: 0.0}, 0
    for name, (c, gts, offs, boxes, gt, norm, info) in assigned.items():
        if name == "tal_640_crowd":
            continue                                                             # minutes in the per-box oracle
        for b in range(c["B"]):
            g5 = gts[int(offs[b]):int(offs[b + 1])].float()
            if g5.shape[0] == 0:
                continue
            if c["atss"]:
                _, _, ts, fg = O.atss_assign(R.anchor_boxes(c["points"], c["stride"]).float(), [h * w for h, w in c["hw"]], boxes[b], g5, c["nc"])
            else:
                _, _, ts, fg = O.tal_assign(c["scores"][b].float(), boxes[b], c["points"], g5, c["nc"], 13, c["alpha"], c["beta"])
            cmp_ = torch.from_numpy(~info[b]["skip"])
            if not torch.equal(fg[cmp_], (gt[b] >= 0)[cmp_]):                     # torch.topk's order among equal values (zero metrics, distance ties) is open:
                differ += 1                                                      # another pick moves the box maxima, so the image's metric is not comparable
                print("  %s image %d: %d anchors differ" % (name, b, int((fg != (gt[b] >= 0))[cmp_].sum())))
                continue
            same = cmp_ & fg & (gt[b] >= 0)
            e = ((ts.sum(-1).double() - norm[b]).abs()[same].max() / norm[b].max()).item() if same.any() else 0.0
            worst[c["atss"]] = max(worst[c["atss"]], e)
    print("fp32 oracle against fp64, worst |d metric| / max metric: TAL %.2e, ATSS %.2e; %d images left out (ties torch.topk leaves open)" % (worst[False], worst[True], differ))
    assert worst[False] <= 2.0 ** -16 and worst[True] <= 2.0 ** -16


def _r32(scores, distri, pts, st, gts, gt, norm, up):
    r64 = R.terms_ref(scores, distri, pts, st, gts, gt, norm, upstream=up)
    r32 = R.terms_ref(scores, distri, pts, st, gts, gt, norm, upstream=up, dtype=torch.float32, want_S=False)
    fin = torch.isfinite(r64["Ss"]) & torch.isfinite(r64["gs"])
    a = ((r32["gs"] - r64["gs"]).abs() / (2.0 ** -24 * r64["Ss"]).clamp_min(1e-300))[fin & (r64["Ss"] > 0)]
    B, A = r64["fg"].shape
    b = ((r32["gd"] - r64["gd"]).abs() / (2.0 ** -24 * r64["Sd"]).clamp_min(1e-300))[(r64["Sd"] > 0) & ~r64["kink"].view(B, A, 1)]
    assert float((r32["gd"][r64["Sd"] == 0]).abs().max()) == 0
    return (float(a.max()) if a.numel() else 0.0), (float(b.max()) if b.numel() else 0.0)


def test_r32_is_below_a_quarter_of_k(assigned):
    """K of loss_ref is 4 x the error of torch's own fp32 autograd on the CPU against fp64, in units of 2^-24 S, over every case of the module (synthetic
    assignments at both upstream gradients, and every assigner case on its fp64 assignment): r32 < K / 4."""
    worst_s = worst_d = 0.0
    arg = ("", "")
    for nc, dt, size, B in R.terms_cases():
        c = R.terms_case(nc, dt, size, B)
        gts, _ = R.host_gts(c["targets"], B, size)
        for up in ((1.0, 1024.0) if B * size < 1000 else (1024.0,)):
            a, b = _r32(c["scores"], c["distri"], c["points"], c["strides"], gts, c["out_gt"], c["out_norm"], up)
            if a > worst_s: worst_s, arg = a, (c["name"], arg[1])
            if b > worst_d: worst_d, arg = b, (arg[0], c["name"])
    for name, (c, gts, offs, boxes, gt, norm, info) in assigned.items():
        a, b = _r32(c["scores"].float(), c["distri"], c["points"], c["stride"], gts, gt, norm, 1.0)
        if a > worst_s: worst_s, arg = a, (name, arg[1])
        if b > worst_d: worst_d, arg = b, (arg[0], name)
    r32 = max(worst_s, worst_d)
    print("r32 = %.2f (scores %.2f in %s, distri %.2f in %s), K = %d" % (r32, worst_s, arg[0], worst_d, arg[1], R.K))
    assert r32 < R.K / 4
    assert R.K == 2 ** math.ceil(math.log2(4 * r32)), "K is 4 r32 rounded up to a power of two: update loss_ref.K and its docstring"


def _old_bar(got, ref):
    """the bar of tests/test_gpu_train.py::test_compute_loss_matches_reference_fixture"""
    return float((got - ref).abs().max()) <= 5e-4 * float(ref.abs().max())


def test_the_per_element_check_rejects_subtly_wrong_results(golden, assigned):
    """Start from the fp64 result rounded to fp32 and apply one change at a time: each must push the per-element check above 1 (or the assignment check
    to a mismatch).  The old bar, max |diff| <= 5e-4 max |grad|, accepts a negative-class gradient scaled by 1.01 — and any error of the negative-class gradients
    below 5e-4 of the largest positive-class one, which is thousands of times their size — so it cannot see an error in the million small gradients next
    to a few large ones; that is the reason for the per-element bound.  (It does reject the dropped -1.5 p log(1 - p) term on this fixture case: at scores
    near 1 that term is a tenth of the largest gradient.  The test prints what the old bar says to each.)  Inputs: case c1 of the nc = 80 reference fixture (no planted values: the comparison with the old bar is
    the one the existing test makes) and the assigner cases `tal_320_a2b2` / `tal_320_f16_zero`."""
    g = golden("loss_cases")
    res, info = _fixture_case(g, 1, False, 80)
    f32 = torch.float32
    gs0, gd0 = res["gs"].float().double(), res["gd"].float().double()
    B, A, nc = gs0.shape
    ratio_s = lambda x: float(R.grad_ratio(x, res["gs"], res["Ss"], f32).max())
    ratio_d = lambda x: R.distri_ratio(x, res, f32)
    assert ratio_s(gs0) <= 1 and ratio_d(gd0)[0] <= 1 and ratio_d(gd0)[1] == 0
    size = int(g["c1_size"])
    pts, st = R.anchors([(size // s, size // s) for s in (8, 16, 32)], (8, 16, 32))
    scores, distri, targets = (torch.from_numpy(g["c1_" + k]) for k in ("scores", "distri", "targets"))
    gts, offs = R.host_gts(targets, B, size)
    boxes = R.decode_f32(distri, pts, st)
    gt, norm, ainfo = R.tal_ref(scores, boxes, pts, gts, offs, 80)
    fgi = torch.nonzero(gt >= 0)
    b, a = fgi[len(fgi) // 2].tolist()
    lab = int(gts[int(gt[b, a]), 0])
    done = []

    def rejected(name, r, old=None):
        done.append(name)
        print("%-58s ratio %.3g%s" % (name, r, "" if old is None else "   old bar %s" % ("accepts" if old else "rejects")))
        assert r > 1, name

    m = gs0.clone(); o = (lab + 1) % nc
    m[b, a, lab], m[b, a, o] = gs0[b, a, o], gs0[b, a, lab]
    rejected("foreground class gradient moved one class over", ratio_s(m))
    n2 = norm.clone(); n2[b, a] += 2.0 ** -10
    r2 = R.terms_ref(scores, distri, pts, st, gts, gt, n2, want_S=False)
    rejected("one anchor's out_norm changed by 2^-10 (gradients)", max(ratio_s(r2["gs"].float().double()), ratio_d(r2["gd"].float().double())[0]))
    assert R.check_assignment(gt, n2, gt, norm, ainfo)[1] > 1
    # DFL left bin off by one: the weight wl of side 0 lands on bin tl - 1 (or tl + 1 at the edge)
    s_ = float(st[a]); u1 = float(gts[int(gt[b, a]), 1]) / s_
    tgt = min(max(float(pts[a, 0]) / s_ - u1, 0.0), 15.99); tl = int(tgt); wl = tl + 1 - tgt
    coef = 0.25 * 0.5 * float(norm[b, a]) / float(res["out"][4]) * wl
    m = gd0.clone(); to = tl - 1 if tl > 0 else tl + 1
    m[b, a, tl] += coef; m[b, a, to] -= coef
    rejected("one anchor's DFL left bin off by one", ratio_d(m)[0])
    neg = torch.nonzero((gt < 0))[7].tolist()
    m = gs0.clone(); m[neg[0], neg[1], 5] *= 1.01
    old_d = _old_bar(m, gs0)
    rejected("one negative score's gradient scaled by 1.01", ratio_s(m), old_d)
    # the gradient through the VariFocal weight of a negative, -1.5 p log(1 - p) * w_cls / target-score sum, taken out of every negative
    l1 = torch.log(1 - scores.double()).clamp_min(-100.0)
    onehot = torch.zeros(B, A, nc, dtype=torch.bool)
    fb, fa = torch.nonzero(gt >= 0, as_tuple=True)
    onehot[fb, fa, gts[gt[fb, fa], 0].long()] = True
    m = torch.where(onehot, res["gs"], res["gs"] + 1.5 * scores.double() * l1 / res["out"][4]).float().double()
    old_e = _old_bar(m, gs0)
    rejected("the -1.5 p log(1 - p) term dropped", ratio_s(m), old_e)
    assert old_d, "the old bar accepts the scaled negative-class gradient"
    small = gs0.abs() < 1e-4 * gs0.abs().max()
    m = torch.where(small, gs0 * 1.5, gs0)
    rejected("every gradient below 1e-4 of the largest scaled by 1.5 (%d)" % int(small.sum()), ratio_s(m), _old_bar(m, gs0))
    assert _old_bar(m, gs0)
    bg = torch.nonzero(gt < 0)[3].tolist()
    m = gd0.clone(); m[bg[0], bg[1], 9] = 1e-30
    r, bad, _ = ratio_d(m)
    rejected("one background distri row non-zero", r)
    assert bad == 1
    # the discrete part, on assigner cases: a shared anchor to the runner-up, and the 13th / 14th pick of a box swapped where their margin is above tau
    c, gts2, offs2, boxes2, gt2, norm2, info2 = assigned["tal_320_a2b2"]
    i0 = info2[0]
    j = int(np.nonzero(i0["multi_margin"] > R.TAU)[0][0])
    m = gt2.clone(); m[0, int(i0["multi"][j])] = int(offs2[0]) + int(i0["second"][j])
    wrong = R.check_assignment(m, norm2, gt2, norm2, info2)[0]
    done.append("shared anchor to the second-best box"); print("%-58s %d anchors differ" % (done[-1], wrong))
    assert wrong == 1
    for box in range(i0["n"]):
        a13, a14 = int(i0["order"][box, 12]), int(i0["order"][box, 13])
        if R.TAU < i0["topk"][box] < 1 and int(gt2[0, a13]) == int(offs2[0]) + box and int(gt2[0, a14]) < 0:
            break
    else:
        raise AssertionError("no box with a clean 13th / 14th pick")
    m = gt2.clone(); m[0, a13] = -1; m[0, a14] = int(offs2[0]) + box
    wrong = R.check_assignment(m, norm2, gt2, norm2, info2)[0]
    done.append("13th and 14th pick swapped (margin %.3g)" % i0["topk"][box]); print("%-58s %d anchors differ" % (done[-1], wrong))
    assert wrong == 2 and len(done) == 9
