"""-m gpu: the label assigners (csrc/tal_assign.hip) and the loss kernels (csrc/loss_terms.hip) against the fp64 restatement of tests/loss_ref.py, at the
class counts, shapes, saturated values and box kinds where they take another path.  Bounds, tau, K and their derivations: the docstring of loss_ref;
tests/test_loss_ref_host.py checks on the CPU that the reference reproduces the fixtures of the reference implementation, that the near-tie cap holds for
every case used here and that the checks reject subtly wrong results.  Every test prints the worst |got - ref| / bound it saw (run with -s).
File:line references are to maf-yolo_amd/csrc/."""
import importlib

import numpy as np
import pytest
import torch

import maf_yolo_amd as M
from maf_yolo_amd import lib

import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
loss_mod = importlib.import_module("maf-yolo_amd.loss")
WEIGHTS = (1.0, 2.5, 0.5)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _decode(distri, pts, st):
    B, A = distri.shape[:2]
    boxes = torch.empty(B, A, 4, dtype=torch.float32, device=DEV)
    lib.check(lib.load().maf_loss_decode(distri.data_ptr(), lib.F16 if distri.dtype == torch.float16 else lib.F32, pts.data_ptr(), st.data_ptr(), B, A, 16,
                                         boxes.data_ptr(), _stream()))
    return boxes


def _check_terms(name, out5, gs, gd, ref, up, dtype, max_kinks=None):
    """forward sums at 5e-5, both gradients per element (the reference is linear in the upstream gradient: scaled, a power of two, exactly)"""
    r_sum = R.check_sums(out5, ref["out"][:out5.numel()])
    r_s = float(R.grad_ratio(gs, ref["gs"] * up, ref["Ss"] * up, dtype).max())
    scaled = dict(ref, gd=ref["gd"] * up, Sd=ref["Sd"] * up)
    r_d, bad_bg, kinks = R.distri_ratio(gd, scaled, dtype)
    print("%-28s upstream %6g: sums %.3f  score gradient %.3f  distri gradient %.3f of the bound (%d kink anchors left out)" % (name, up, r_sum, r_s, r_d, kinks))
    assert r_sum <= 1, "sums"
    assert r_s <= 1, "score gradient"
    assert r_d <= 1 and bad_bg == 0, "distri gradient (%d background rows not zero)" % bad_bg
    assert kinks <= (0.001 * ref["fg"].numel() + 1 if max_kinks is None else max_kinks)
    return r_s, r_d


def _terms(c, ups=(1.0, 1024.0)):
    B, A, nc = c["scores"].shape
    dtype = c["scores"].dtype
    pts, st = c["points"].to(DEV).contiguous(), c["strides"].to(DEV).contiguous()
    targets = c["targets"].to(DEV)
    gts, gt_img, offs, T = loss_mod._targets_on_device(targets, B, c["size"], DEV)
    R.check_targets(gts, gt_img, offs, T, c["targets"], B, c["size"])
    og, on = c["out_gt"].to(DEV).contiguous(), c["out_norm"].to(DEV).contiguous()
    ref = R.terms_ref(c["scores"], c["distri"], c["points"], c["strides"], gts.cpu(), c["out_gt"], c["out_norm"], WEIGHTS, 1.0)
    for up in ups:
        s = c["scores"].to(DEV).requires_grad_(True); d = c["distri"].to(DEV).requires_grad_(True)
        out = loss_mod._FusedTerms.apply(s, d, pts, st, gts, og, on, 16, WEIGHTS)
        (out[0] * up).backward()
        assert s.grad.dtype == dtype and d.grad.dtype == dtype
        _check_terms(c["name"], out.detach(), s.grad, d.grad, ref, up, dtype, 0 if c["size"] == 64 else None)    # 64 x 64: no anchor may drop out as a kink
    assert not bool(ref["fg"].any()) or min(ref["clips"]) > 0, "DFL targets clipped at 0 / 15.99: %s" % (ref["clips"],)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("nc", R.TERMS_NC)
def test_loss_terms_at_every_class_count_with_a_synthetic_assignment(nc, dtype):
    """maf_loss_terms, forward and gradient (upstream 1 and 1024), on a frozen synthetic assignment at 64 x 64 (A = 84), B = 1 and B = 3.
      * loss_terms.hip:247,257,261 — nc = 1, 3, 20, 81 take loss_cls_kernel<T, 1, *>, the scalar path; nc = 8, 80 the 8-wide one.
      * :110-124 — the positive classes cycle through class 0, class nc - 1 and 9 j mod nc (j = 1..7): for nc = 8 and 80 one in each of the 8 vector lanes, and
        in the first and the last vector of an anchor's row.
      * :104,107,116,120 — planted scores exactly 0, exactly 1 (the -100 log clamps, the 1e-12 floor of p (1 - p); fp16 gradients overflow to the same
        infinity), 2^-24 and 1 - 2^-11, on negatives and on positive classes.
      * :198 — row 1 of every image is a corner box most of its anchors lie outside of (the DFL target clips at 0), row 2 a box five times the image (clips
        at 15.99 from every anchor; the whole image, row 0, clips from stride-8 anchors only at 320 x 320, in the next test); both counts are asserted from
        the reference.  Planted distri rows: all mass on bin 0 (zero-size predicted box), on bin 16, and +-30 (fp16: +-20) logits.
      * :166-168 — anchors 16..31 are all background (a wave with no foreground; its lanes compute on anchor 0), and at B = 3 no 64-anchor tile is free of a
        planted anchor (the 320 x 320 test has the empty tile); foreground at the first and last anchor of every image and of a 64-anchor tile (63, 64, 127).
      * B * A = 84 and 252 are no multiple of 64: the last tile of loss_box_kernel is partial (:165).  The partial last tile of loss_decode_kernel (:39,45)
        is checked by test_assigners_against_fp64, which compares the decoded boxes with decode_ref.
      * out_norm holds 1.0 and 2^-20."""
    for B in (1, 3):
        c = R.terms_case(nc, dtype, 64, B)
        assert (c["out_gt"].reshape(-1)[16:32] < 0).all() and all(int(c["out_gt"].reshape(-1)[f]) >= 0 for f in c["forced"])
        lab = c["targets"][:, 1].long()[c["out_gt"][c["out_gt"] >= 0].long()]
        if nc % 8 == 0:
            assert set((lab % 8).tolist()) == set(range(8)) and 0 in lab.tolist() and nc - 1 in lab.tolist()
        _terms(c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_loss_terms_grid_stride_loops_wrap(dtype):
    """320 x 320, B = 32, nc = 80: B * A = 67200 anchors > 1024 tiles of 64 and B * A * nc / 8 = 672000 vectors > 1024 x 256: both grid-stride loops
    (loss_terms.hip:94 and :163) wrap — the smallest shape that wraps them.  A whole 64-anchor tile has no foreground (:166)."""
    c = R.terms_case(80, dtype, 320, 32)
    NA = c["out_gt"].numel()
    assert NA > 65536 and NA * 80 // 8 > 262144 and c["empty_tile"] >= 0
    assert (c["out_gt"].reshape(-1)[c["empty_tile"] * 64:c["empty_tile"] * 64 + 64] < 0).all()
    _terms(c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_loss_terms_all_background_batch(dtype):
    """No foreground anchor: the target-score sum is 0, cls and the total are inf, the box terms 0 (loss_terms.hip:148-149), the distri gradient exactly 0
    (no wave passes :166) and the score gradient the same inf / NaN pattern as the reference's division by 0."""
    c = R.background_case(dtype)
    ref = _terms(c)
    o = ref["out"]
    assert torch.isinf(o[0]) and torch.isinf(o[3]) and o[1] == 0 and o[2] == 0 and o[4] == 0 and float(ref["gd"].abs().max()) == 0


@pytest.mark.parametrize("name", R.ASSIGN_NAMES)
def test_assigners_against_fp64(name):
    """maf_tal_targets against targets_ref, maf_loss_decode against decode_ref (per element, |got - ref| <= ulp + K_DEC 2^-24 S: loss_terms.hip:39,45, the
    partial last tile, at B * A = 168, 378, 120, 174: no multiple of 64, in fp32 and — the cases of loss_ref.F16_DISTRI — fp16 logits), then maf_tal_assign /
    maf_atss_assign against tal_ref / atss_ref on the kernel's own rows and boxes, then the fused fp32 loss on the kernel's assignment against terms_ref (the
    two halves joined).  Every case but tal_T1500 (random boxes on a 2^-12 lattice) and tal_640_crowd (a lattice of duplicated boxes plus 3 random ones)
    holds the box kinds of loss_ref._kinds: zero width,
    thinner than a cell, wholly outside, the whole image, partly outside, exact duplicates (all their anchors are claimed twice at equal IoU: first row),
    nested with one centre; ATSS also an all-zero row (tal_assign.hip:311 gvalid), a centre in each corner cell (the clamped 9 x 9 window, :317-319) and a
    centre exactly on a cell corner with fp32-exact edges (exact distance ties, :334: lowest anchor first).
      tal_64_nc1        64 x 64 (A = 84), nc = 1, fp32
      tal_96_nc3_f16    96 x 96 (A = 189), nc = 3, fp16 scores, alpha 0.5 / beta 2.5: pow_slow (tal_assign.hip:51,61)
      tal_320_f16_zero  320 x 320, nc = 80, fp16 scores exactly 0 inside a box that covers the first anchors, only the last 5 of its inside anchors positive: the
                        zero-metric fill (:191-205) takes 8 zero-score anchors that lie inside; asserted from the reference, here and for tal_1level_A60
      tal_320_a2b2      alpha 2 / beta 2: the whole-exponent path of pow_pos (:56-59) for both powers
      tal_nonsquare     level_hw (5,12), (3,6), (2,3) (:73, :402-414), also through task_aligned_assign(level_hw=...)
      tal_1level_A60    one level (5,12): A = 60 < 64 anchors (:196 lanes past A) with exact-zero fp16 scores
      tal_4levels       strides 8, 16, 32, 64 (4 levels: every branch of the level selects, :144-151)
      tal_T1500         1500 ungrouped labels over B = 4 (:386-391 with T > 1024 threads), 60 with image id -1, B, B + 3 dropped (:370, :105; offsets end at 1440)
      tal_640_crowd     640 x 640, image 0 with 600 disjoint boxes listed twice: 1200 > kGtL (:237 reads rows past 1024 from memory) and 7600 > kMulti anchors
                        claimed twice (:246 in-place best_box); duplicates resolve to the first row.  Both thresholds asserted from the reference.
      atss_96_nc3       96 x 96: the last level is 3 x 3, the smallest the entry accepts
      atss_320          320 x 320, 67 boxes
      atss_nonsquare    level_hw (5,12), (3,6), (3,3)
      atss_ungrouped    B = 3, labels shuffled, three rows with image ids -1, B, B + 3 dropped (:308)"""
    c = R.assign_case(name)
    B, size, nc = c["B"], c["size"], c["nc"]
    pts, st = c["points"].to(DEV).contiguous(), c["stride"].to(DEV).contiguous()
    levels = loss_mod._levels(c["hw"], c["strides"], 0.5)
    targets = c["targets"].to(DEV)
    gts, gt_img, offs, T = loss_mod._targets_on_device(targets, B, size, DEV)
    n = R.check_targets(gts, gt_img, offs, T, c["targets"], B, size)
    distri = c["distri"].to(DEV)
    boxes = _decode(distri, pts, st)
    dref, dS = R.decode_ref(c["distri"], c["points"], c["stride"])
    r_dec = float(R.decode_ratio(boxes, dref, dS).max())
    print("%-18s decode (%s logits, B * A = %d): %.3f of the bound" % (name, "fp16" if distri.dtype == torch.float16 else "fp32", B * pts.shape[0], r_dec))
    assert r_dec <= 1, "decoded boxes"
    distri = distri.float()
    scores = c["scores"].to(DEV)
    if c["atss"]:
        out_gt, out_norm = loss_mod._assign_atss(boxes, pts, levels, gts, gt_img, offs, T)
    else:
        out_gt, out_norm = loss_mod._assign(scores, boxes, pts, levels, gts, gt_img, offs, T, 13, c["alpha"], c["beta"])
    gts_c = gts.cpu()[:n]
    ref_gt, ref_norm, info = R.assign_ref(c, gts_c, offs.cpu(), boxes.cpu())
    nb, near = R.near_share(info)
    wrong, rel, bg = R.check_assignment(out_gt, out_norm, ref_gt, ref_norm, info)
    print("%-18s boxes %d (near-tied %d), foreground %d, multiply-claimed %s: %d anchors differ, normalised metric %.3f of 2^-16 relative" %
          (name, nb, near, int((ref_gt >= 0).sum()), [i["n_multi"] for i in info], wrong, rel))
    assert near <= R.NEAR_CAP * nb and (nb >= 50 or near == 0)
    assert wrong == 0 and bg == 0 and rel <= 1
    assert int((ref_gt >= 0).sum()) > 0
    if name in R.ZERO_FILL:
        assert info[0]["zero_score_inside"] > 0, "the zero-metric fill is not reached through zero scores"
    if name == "tal_640_crowd":
        assert info[0]["n"] > R.K_GTL and info[0]["n_multi"] > R.K_MULTI and int(out_gt[0].max()) < 600
    if name == "atss_ungrouped":
        assert int(offs[-1]) == c["targets"].shape[0] - 3
    if name == "tal_T1500":
        assert int(offs[-1]) == 1440 and int(out_gt.max()) < 1440
    if name == "tal_nonsquare":
        labels, tb, ts, fg = M.task_aligned_assign(scores, boxes, pts, targets, B, size, nc, 13, c["alpha"], c["beta"], level_hw=c["hw"], strides=c["strides"])
        assert torch.equal(fg.cpu(), ref_gt >= 0) and torch.equal(ts.sum(-1), out_norm)
        assert torch.equal(labels.cpu()[ref_gt >= 0], gts_c[:, 0].long()[ref_gt[ref_gt >= 0]])
    # the fused loss (fp32) on the kernel's own assignment
    s = scores.float().requires_grad_(True); d = distri.clone().requires_grad_(True)
    feats = [torch.zeros(B, 8, h, w, device=DEV) for h, w in c["hw"]]
    crit = M.ComputeLoss(fpn_strides=c["strides"], num_classes=nc, ori_img_size=size, fused=True)
    loss, items = crit((feats, s, d), targets, 5, 1, assignment=(out_gt, out_norm))
    loss.backward()
    ref = R.terms_ref(scores.float(), distri, c["points"], c["stride"], gts_c, out_gt, out_norm, WEIGHTS, 1.0)
    _check_terms(name, torch.cat([loss.detach().reshape(1), items]), s.grad, d.grad, ref, 1.0, torch.float32)


def _nc_case(golden, ci):
    g = golden("loss_cases_nc")
    size = int(g["c%d_size" % ci])
    return g, size, [(size // s, size // s) for s in (8, 16, 32)], int(g["c%d_nc" % ci])


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_compute_loss_matches_reference_fixture_at_other_class_counts(golden, ci, fused):
    """The reference's own ComputeLoss (tools/make_golden_loss.py, loss_cases_nc.npz) at num_classes 1, 3, 20 and 20 with a crowded image (60 boxes,
    duplicates and nesting), sizes 96 and 160, task-aligned assigner: the bars of test_gpu_train.py::test_compute_loss_matches_reference_fixture."""
    g, size, hw, nc = _nc_case(golden, ci)
    s = torch.from_numpy(g["c%d_scores" % ci]).to(DEV).requires_grad_(True)
    d = torch.from_numpy(g["c%d_distri" % ci]).to(DEV).requires_grad_(True)
    feats = [torch.zeros(s.shape[0], 8, h, w, device=DEV) for h, w in hw]
    crit = M.ComputeLoss(num_classes=nc, ori_img_size=size, fused=fused)
    loss, items = crit((feats, s, d), torch.from_numpy(g["c%d_targets" % ci]).to(DEV), 5, 1)
    want = float(g["c%d_loss" % ci])
    assert abs(loss.item() - want) <= 5e-5 * abs(want)
    assert np.allclose(items.cpu().numpy(), g["c%d_items" % ci], rtol=5e-5, atol=1e-6)
    loss.backward()
    gs, gd = g["c%d_gscores" % ci], g["c%d_gdistri" % ci]
    assert np.abs(s.grad.cpu().numpy() - gs).max() <= 5e-4 * np.abs(gs).max()
    assert np.abs(d.grad.cpu().numpy() - gd).max() <= 5e-4 * np.abs(gd).max()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_compute_loss_warmup_atss_matches_reference_fixture_at_other_class_counts(golden, ci, fused):
    """The a* keys of loss_cases_nc.npz: epoch 0 -> ATSS, the bars of test_gpu_train.py::test_compute_loss_warmup_atss_matches_reference_fixture."""
    g, size, hw, nc = _nc_case(golden, ci)
    s = torch.from_numpy(g["c%d_scores" % ci]).to(DEV).requires_grad_(True)
    d = torch.from_numpy(g["c%d_distri" % ci]).to(DEV).requires_grad_(True)
    feats = [torch.zeros(s.shape[0], 8, h, w, device=DEV) for h, w in hw]
    crit = M.ComputeLoss(num_classes=nc, ori_img_size=size, fused=fused)
    loss, items = crit((feats, s, d), torch.from_numpy(g["c%d_targets" % ci]).to(DEV), 0, 1)
    want = float(g["a%d_loss" % ci])
    assert abs(loss.item() - want) <= 5e-5 * abs(want)
    assert np.allclose(items.cpu().numpy(), g["a%d_items" % ci], rtol=5e-5, atol=1e-6)
    loss.backward()
    gs, gd = g["a%d_gscores" % ci].astype(np.float32), g["a%d_gdistri" % ci]
    assert np.abs(s.grad.cpu().numpy() - gs).max() <= 1e-3 * np.abs(gs).max()
    assert np.abs(d.grad.cpu().numpy() - gd).max() <= 5e-4 * np.abs(gd).max()
