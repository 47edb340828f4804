"""fp64 restatement of the training loss on the CPU: label preprocessing, the task-aligned and the ATSS assigner, and the loss terms with their gradients —
the reference of tests/test_gpu_loss_edges.py for csrc/tal_assign.hip and csrc/loss_terms.hip, tied to the reference's own ComputeLoss by
tests/test_loss_ref_host.py (the fixtures of tools/make_golden_loss.py).  Nothing here imports the package: numpy and torch on the CPU only.

Rules: oracle/maf_oracle.py tal_assign / atss_assign (yolov6/assigners/tal_assigner.py, atss_assigner.py, assigner_utils.py), vectorised over the boxes of an
image.  Exact ties follow what the kernels document: lowest anchor first in a top-k (a stable sort), first box on equal IoU (argmax), zero metrics in anchor
order from anchor 0 (the same stable sort: torch.topk leaves the order among equal values open, the kernels do not).

Discrete outputs and tau.  The kernels decide in fp32.  An fp32 IoU carries about 8 roundings (4 subtractions / min / max, 2 products, the union, the division):
8 * 2^-24 = 2^-21; its sixth power 6 * 2^-21 = 2^-18.4; two metrics compared, each times the score power and with the rounding of the power itself: times 4 ->
tau = 2^-16 relative.  A decision whose fp64 margin is positive and below tau is near-tied: the anchors it touches (the candidates of the box, every anchor
assigned to a box that shares one of them) are left out of the comparison.  A margin of exactly 0 is a tie by construction (duplicated boxes, centres on cell
corners at fp32-exact coordinates, zero metrics) and is compared.  A metric that is positive in fp64 and below the fp32 normal range counts as near-tied
(fp32 may flush it to the zero-metric rule).  Margins returned per image in `info`:
  * topk     per box: (m_k - m_k+1) / m_k of the last kept and first rejected positive metric (ATSS: per level (d_k+1 - d_k) / d_k+1 of the distances);
  * thr      ATSS: |IoU - threshold| / threshold of every candidate;
  * multi    per multiply-claimed anchor: (best - second) / best IoU over all boxes of the image;
  * inside   per (box, anchor): |dmin - eps| / |dmin|.  The reference consumes the kernel's own fp32 rows and anchor centres; an fp32 difference of two
             fp32 numbers is correctly rounded, zero exactly when they are equal, and a non-zero one is at least an ulp of the smaller operand (anchor
             centres are >= 4), far above eps = 1e-9: the fp32 test equals the exact one unless dmin itself is within tau of eps.
Normalised metric / IoU: |got - ref| <= 2^-16 |ref| on compared anchors (the metric, its maximum and the IoU maximum each carry 2^-18.4 or less), background
exactly 0.  The fp32 CPU oracle (oracle.maf_oracle.tal_assign / atss_assign) against this module on the cases below: worst |fp32 - fp64| = 1.4e-6 of the
case's maximum (TAL), 1.0e-7 (ATSS); tests/test_loss_ref_host.py prints both.

Loss terms (loss.py:_torch_terms = yolov6/models/loss.py:150-267 for a frozen assignment): float64 autograd, F.binary_cross_entropy with its -100 log clamp
and the 1e-12 floor of p (1 - p) in its backward.  fp16 inputs are upcast exactly.  The five sums: relative 5e-5 (all addends non-negative: S = |ref|), the
same infinities where the target-score sum is 0.  Gradients per element: |got - ref| <= ulp_T(ref) + K * 2^-24 * S, S = the gradient's expression with every
term taken in absolute value, plus the sensitivity of log(1 - p), log p and 1 / (p (1 - p)) to one fp32 rounding of 1 - p (absolute 2^-24 on the log: near
p = 0 the fp32 value of 1 - p dominates the error, and the reference's own fp32 arithmetic has it too), and of the softmax to the rounding of z - max
(relative |z - max| 2^-24 on a bin's probability).
K is not fitted to the kernels: the same formulas evaluated with torch fp32 autograd on the CPU on every case of this module give

    r32 = max |fp32 - fp64| / (2^-24 S) = 3.41       (scores 2.51, distri 3.41, both in `terms_nc80_f32_B32_320`; printed by tests/test_loss_ref_host.py)
    K   = 4 * r32 rounded up to a power of two = 16

(the factor 4: the kernels' v_log_f32 / v_rcp_f32 are about 1 ulp instead of correctly rounded, and their expf / softmax order is their own).  The host test
recomputes r32 and asserts r32 < K / 4.  One comparison uses more than K: the reference fixtures' gradients (tests/test_loss_ref_host.py) come from the
reference's own fp32 assignment, whose normalised metric and target-score sum are each within 2^-16 relative of the fp64 ones (above); every gradient term is
linear in the one and inverse in the other, so that comparison alone allows K 2^-24 S + 3 * 2^-16 S.  It is derived, not fitted: the kernels are never compared
with it, they get the reference on their own assignment and K.  The decode (decode_ref) has its own constant from the same rule: torch's fp32 decode on the
assigner cases gives r32 = 1.19, K_DEC = 8.  Where the fp64 gradient overflows the tensor's dtype (saturated fp16 scores) the same infinity is required; every
background row of the distri gradient must be exactly 0.  The GIoU gradient is discontinuous where a predicted coordinate crosses the target's (min / max) or
the overlap crosses 0 (clamp): an anchor where one of these gaps is non-zero and below tau relative is a near-tied decision too (`kink`) and its distri rows
are left out; exact equality takes the 0.5 / 0.5 sub-gradient in autograd and in the kernel alike and is compared.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

TAU = 2.0 ** -16
K = 16
K_DEC = 8             # the decode kernel: 4 x r32 of torch's fp32 decode against decode_ref (see the module docstring)
NEAR_CAP = 0.02            # near-tied decisions may involve at most 2 % of a case's boxes (none below 50 boxes)
K_GTL, K_MULTI = 1024, 4096  # csrc/tal_assign.hip kGtL / kMulti
F32_TINY = 2.0 ** -120
R1 = 17


def ulp(x, dtype):
    """Spacing of `dtype` (fp16 / fp32) at |x|, the subnormal spacing below the normal range."""
    lo, m = (2.0 ** -14, 10) if dtype == torch.float16 else (2.0 ** -126, 23)
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(lo))) - m)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# anchors and label preprocessing
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def anchors(level_hw, strides, offset=0.5):
    """anchor centres [A,2] in pixels and the stride of every anchor [A], fp32 (anchor_generator.py:26-53)"""
    pts, st = [], []
    for (h, w), s in zip(level_hw, strides):
        ys = (torch.arange(h, dtype=torch.float32) + offset) * s
        xs = (torch.arange(w, dtype=torch.float32) + offset) * s
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        pts.append(torch.stack([xx, yy], -1).reshape(-1, 2))
        st.append(torch.full((h * w,), float(s)))
    return torch.cat(pts), torch.cat(st)


def anchor_boxes(points, strides, cell_size=5.0):
    half = (cell_size * 0.5) * strides.double()[:, None]
    return torch.cat([points.double() - half, points.double() + half], -1)


def targets_ref(targets, B, img_size):
    """labels [T,6] = (image, class, cx, cy, w, h) normalised -> (rows [n,5] = (class, x1, y1, x2, y2) pixels grouped by image in their original order,
    image of every row [n], offsets [B+1], index of every kept row [n]); rows whose image id is outside [0, B) are dropped (loss.py:179-188)."""
    t = targets.detach().double().cpu().reshape(-1, 6)
    ids = t[:, 0]
    ok = (ids >= 0) & (ids < B)
    im = torch.where(ok, ids.floor(), torch.full_like(ids, -1)).long()
    keep = torch.nonzero(ok).reshape(-1)
    keep = keep[torch.sort(im[keep], stable=True)[1]]
    r = t[keep]
    cx, cy, w, h = r[:, 2] * img_size, r[:, 3] * img_size, r[:, 4] * img_size, r[:, 5] * img_size
    rows = torch.stack([r[:, 1], cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    offs = torch.zeros(B + 1, dtype=torch.long)
    offs[1:] = torch.cumsum(torch.bincount(im[keep], minlength=B), 0)
    return rows, im[keep], offs, keep


def check_targets(gts, gt_img, offs, T_in, targets, B, img_size):
    """the device preprocessing against targets_ref: offsets, image ids and row order equal, coordinates to one fp32 ulp of img_size (hipcc may contract
    cx * size - w * size / 2, so bit equality is not required)"""
    rows, im, o, keep = targets_ref(targets, B, img_size)
    n = rows.shape[0]
    assert torch.equal(offs.cpu().long(), o), "offsets"
    assert torch.equal(gt_img.cpu().long()[:n], im), "image of every row"
    got = gts.detach().cpu().double()[:n]
    assert torch.equal(got[:, 0], rows[:, 0]), "labels / row order"
    tol = float(ulp(torch.tensor(float(img_size)), torch.float32))
    err = (got[:, 1:] - rows[:, 1:]).abs().max().item() if n else 0.0
    assert err <= tol, "coordinates off by %.3g (one ulp of the image size: %.3g)" % (err, tol)
    return n


def decode_f32(distri, points, strides):
    """loss.py:190-193 in fp32 on the CPU: the pixel boxes the assigner ranks (host stand-in of loss_decode_kernel for the near-tie census)"""
    B, A = distri.shape[:2]
    d = F.softmax(distri.float().view(B, A, 4, R1), -1).matmul(torch.arange(R1, dtype=torch.float32))
    ps = points / strides[:, None]
    return torch.cat([ps - d[..., :2], ps + d[..., 2:]], -1) * strides[:, None]


def decode_ref(distri, points, strides):
    """loss.py:190-193 in fp64 (fp16 / fp32 logits upcast exactly) -> (pixel boxes [B,A,4], S).  d = sum_k q_k k over the softmax q of a side's 17 logits,
    box = (centre / stride -/+ d) * stride.  S takes every term in absolute value, with the sensitivity of a bin's probability to the fp32 rounding of
    z - max (relative |z - max| 2^-24) and of the normalising sum: S = (|centre / stride| + sum_k q_k (1 + |z_k - max|) (k + d)) * stride.
    Bound of loss_decode_kernel: |got - ref| <= ulp_fp32(ref) + K_DEC 2^-24 S (decode_ratio)."""
    B, A = distri.shape[:2]
    z = distri.detach().cpu().double().view(B, A, 4, R1)
    ks = torch.arange(R1, dtype=torch.float64)
    q = F.softmax(z, -1)
    d = (q * ks).sum(-1)
    Sd = (q * (1 + (z - z.max(-1, keepdim=True)[0]).abs()) * (ks + d.unsqueeze(-1))).sum(-1)
    st = strides.double()[:, None]
    ps = points.double() / st
    ref = torch.cat([ps - d[..., :2], ps + d[..., 2:]], -1) * st
    S = (torch.cat([ps, ps], -1).abs() + Sd) * st
    return ref, S


def decode_ratio(got, ref, S, k=None):
    k = K_DEC if k is None else k
    return (got.detach().cpu().double() - ref).abs() / (ulp(ref, torch.float32) + k * 2.0 ** -24 * S)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# assigners
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _pair_iou(g, p, eps):
    """assigner_utils.py:68-89: g [n,4] x p [A,4] -> [n,A]"""
    ix = (np.minimum(g[:, None, 2], p[None, :, 2]) - np.maximum(g[:, None, 0], p[None, :, 0])).clip(0)
    iy = (np.minimum(g[:, None, 3], p[None, :, 3]) - np.maximum(g[:, None, 1], p[None, :, 1])).clip(0)
    inter = ix * iy
    a1 = (g[:, 2] - g[:, 0]).clip(0) * (g[:, 3] - g[:, 1]).clip(0)
    a2 = (p[:, 2] - p[:, 0]).clip(0) * (p[:, 3] - p[:, 1]).clip(0)
    return inter / (a1[:, None] + a2[None] - inter + eps)


def _dmin(g, pts):
    return np.minimum(np.minimum(pts[None, :, 0] - g[:, None, 0], pts[None, :, 1] - g[:, None, 1]),
                      np.minimum(g[:, None, 2] - pts[None, :, 0], g[:, None, 3] - pts[None, :, 1]))


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def _resolve(mask, ov_all, near_box, cand_sets):
    """select_highest_overlaps (assigner_utils.py:46-66): mask [n,A] bool -> assigned box per anchor or -1, multiply-claimed anchors, their margins, runner-up"""
    n, A = mask.shape
    cnt = mask.sum(0)
    gt = np.where(cnt > 0, mask.argmax(0), -1)
    multi = np.nonzero(cnt > 1)[0]
    second = np.zeros(0, dtype=np.int64)
    margin = np.zeros(0)
    if multi.size:
        o = ov_all[:, multi]
        best = o.argmax(0)                                                      # first maximum
        bv = o[best, np.arange(multi.size)]
        o2 = o.copy()
        o2[best, np.arange(multi.size)] = -1.0
        second = o2.argmax(0)
        sv = o2[second, np.arange(multi.size)]
        margin = np.where(bv > 0, (bv - sv) / np.where(bv > 0, bv, 1.0), 0.0)
        gt[multi] = best
        for j in np.nonzero((margin > 0) & (margin < TAU))[0]:
            near_box[best[j]] = near_box[second[j]] = True
            cand_sets.append(np.array([multi[j]]))
    return gt, multi, margin, second


def _skip_mask(n, A, gt, near_box, touched, cands):
    """anchors left out of the comparison: those a near-tied decision touches, and every anchor assigned to a box that shares one of them"""
    skip = np.zeros(A, dtype=bool)
    if not near_box.any():
        return skip
    t = np.zeros(A, dtype=bool)
    for c in touched:
        t[c[c >= 0]] = True
    hit = near_box.copy()
    for g in range(n):
        c = cands[g]
        if t[c[c >= 0]].any():
            hit[g] = True
    skip |= t
    skip |= (gt >= 0) & hit[np.clip(gt, 0, None)]
    return skip


def tal_ref(scores, boxes, points, gts, offs, nc, topk=13, alpha=1.0, beta=6.0, eps=1e-9):
    """scores [B,A,nc], boxes [B,A,4] xyxy pixels, points [A,2], gts [T,5] (class, xyxy) sorted by image, offs [B+1]
    -> (row of the assigned box per anchor or -1 [B,A] int64, normalised alignment metric [B,A] float64, info per image)."""
    sc, bx, pts, gt_all = _np(scores), _np(boxes), _np(points), _np(gts)
    B, A = sc.shape[:2]
    offs = [int(v) for v in offs]
    out_gt = np.full((B, A), -1, dtype=np.int64)
    out_norm = np.zeros((B, A))
    info = []
    for b in range(B):
        g0, n = offs[b], offs[b + 1] - offs[b]
        if n == 0:
            info.append(dict(n=0, near=0, skip=np.zeros(A, dtype=bool), n_multi=0, order=np.zeros((0, topk + 1), dtype=np.int64), zero_inside=0, zero_score_inside=0,
                             topk=np.zeros(0), multi=np.zeros(0, dtype=np.int64), multi_margin=np.zeros(0), second=np.zeros(0, dtype=np.int64)))
            continue
        g = gt_all[g0:g0 + n]
        lab = g[:, 0].astype(np.int64)
        ov = _pair_iou(g[:, 1:], bx[b], eps)
        metric = sc[b][:, lab].T ** alpha * ov ** beta                              # tal_assigner.py:96-111
        dm = _dmin(g[:, 1:], pts)
        inside = dm > eps                                                           # assigner_utils.py:25-44
        near_box = ((dm != 0) & (np.abs(dm - eps) < TAU * np.abs(dm))).any(1)
        pm = metric * inside
        near_box |= ((pm > 0) & (pm < F32_TINY)).any(1)
        kk = min(topk + 1, A)
        order = np.argsort(-pm, axis=1, kind="stable")[:, :kk]                      # descending, lowest anchor among equals, zeros from anchor 0
        vals = np.take_along_axis(pm, order, 1)
        margin = np.ones(n)
        if kk > topk:
            last, nxt = vals[:, topk - 1], vals[:, topk]
            margin = np.where(nxt > 0, (last - nxt) / np.where(last > 0, last, 1.0), np.where(last > 0, 1.0, 0.0))
            near_box |= (nxt > 0) & (margin > 0) & (margin < TAU)
        cand = order[:, :topk]
        mask = np.zeros((n, A), dtype=bool)
        np.put_along_axis(mask, cand, True, 1)
        mask &= inside
        # zero-metric picks that count because they lie inside the box, and those among them whose score is exactly 0 (not a zero IoU)
        zero_pick = (vals[:, :topk] == 0) & np.take_along_axis(inside, cand, 1)
        zero_score = zero_pick & (np.take_along_axis(sc[b][:, lab].T, cand, 1) == 0)
        touched = [order[i] for i in np.nonzero(near_box)[0]]
        gt, multi, mmargin, second = _resolve(mask, ov, near_box, touched)
        fg = gt >= 0
        gi = np.clip(gt, 0, None)
        m_a = np.where(fg, metric[gi, np.arange(A)], 0.0)                           # tal_assigner.py:66-71 (the metric is not masked by `inside` there)
        o_a = np.where(fg, ov[gi, np.arange(A)], 0.0)
        max_m, max_o = np.zeros(n), np.zeros(n)
        np.maximum.at(max_m, gi[fg], m_a[fg])
        np.maximum.at(max_o, gi[fg], o_a[fg])
        out_gt[b] = np.where(fg, g0 + gt, -1)
        out_norm[b] = np.where(fg, m_a * max_o[gi] / (max_m[gi] + eps), 0.0)
        info.append(dict(n=n, near=int(near_box.sum()), skip=_skip_mask(n, A, gt, near_box, touched, cand), n_multi=int(multi.size), order=order,
                         topk=margin, multi=multi, multi_margin=mmargin, second=second, zero_inside=int(zero_pick.sum()), zero_score_inside=int(zero_score.sum())))
    return torch.from_numpy(out_gt), torch.from_numpy(out_norm), info


def atss_ref(anchor_boxes_, n_level, boxes, gts, offs, topk=9):
    """anchor_boxes_ [A,4], n_level = anchors per level, boxes [B,A,4] predicted xyxy pixels -> (assigned row or -1, IoU of the predicted box with it, info)"""
    ab, bx, gt_all = _np(anchor_boxes_), _np(boxes), _np(gts)
    B, A = bx.shape[:2]
    offs = [int(v) for v in offs]
    out_gt = np.full((B, A), -1, dtype=np.int64)
    out_norm = np.zeros((B, A))
    ac = np.stack([(ab[:, 0] + ab[:, 2]) / 2.0, (ab[:, 1] + ab[:, 3]) / 2.0], 1)
    area2 = (ab[:, 2] - ab[:, 0]) * (ab[:, 3] - ab[:, 1])
    info = []
    for b in range(B):
        g0, n = offs[b], offs[b + 1] - offs[b]
        if n == 0:
            info.append(dict(n=0, near=0, skip=np.zeros(A, dtype=bool), n_multi=0, multi=np.zeros(0, dtype=np.int64), multi_margin=np.zeros(0),
                             second=np.zeros(0, dtype=np.int64), topk=np.zeros(0), thr=np.zeros(0)))
            continue
        gb = gt_all[g0:g0 + n, 1:]
        valid = gb.sum(-1) > 0                                                      # loss.py:77 mask_gt
        area1 = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        w = (np.minimum(gb[:, None, 2], ab[None, :, 2]) - np.maximum(gb[:, None, 0], ab[None, :, 0])).clip(0)
        h = (np.minimum(gb[:, None, 3], ab[None, :, 3]) - np.maximum(gb[:, None, 1], ab[None, :, 1])).clip(0)
        inter = w * h
        ov = inter / np.maximum(area1[:, None] + area2[None] - inter, 1e-6)        # iou2d_calculator.bbox_overlaps, eps 1e-6
        gc = np.stack([(gb[:, 0] + gb[:, 2]) / 2.0, (gb[:, 1] + gb[:, 3]) / 2.0], 1)
        dist = np.sqrt(((gc[:, None] - ac[None]) ** 2).sum(-1))
        near_box = np.zeros(n, dtype=bool)
        cand, dmargin, start = [], np.ones(n), 0
        for nl in n_level:                                                          # atss_assigner.py:89-116
            k = min(topk, nl)
            o = np.argsort(dist[:, start:start + nl], axis=1, kind="stable")[:, :min(k + 1, nl)]
            if o.shape[1] > k:
                dk, dn = np.take_along_axis(dist[:, start:start + nl], o[:, k - 1:k + 1], 1).T
                m = np.where(dn > 0, (dn - dk) / np.where(dn > 0, dn, 1.0), 0.0)
                dmargin = np.minimum(dmargin, m)
                near_box |= (m > 0) & (m < TAU)
            cand.append(o[:, :k] + start)
            start += nl
        cand = np.concatenate(cand, 1)
        cov = np.take_along_axis(ov, cand, 1)                                       # atss_assigner.py:118-137
        thr = cov.mean(1) + cov.std(1, ddof=1)
        tm = np.abs(cov - thr[:, None]) / np.where(thr > 0, thr, 1.0)[:, None]
        near_box |= ((tm > 0) & (tm < TAU)).any(1)
        dm = _dmin(gb, ac)
        near_box |= ((dm != 0) & (np.abs(dm - 1e-9) < TAU * np.abs(dm))).any(1)
        pos = np.zeros((n, A), dtype=bool)
        np.put_along_axis(pos, cand, cov > thr[:, None], 1)
        mask = pos & (dm > 1e-9) & valid[:, None]
        touched = [cand[i] for i in np.nonzero(near_box)[0]]
        gt, multi, mmargin, second = _resolve(mask, ov, near_box, touched)
        fg = gt >= 0
        gi = np.clip(gt, 0, None)
        iou_pd = _pair_iou(gb, bx[b], 1e-9)                                         # atss_assigner.py:80-84
        out_gt[b] = np.where(fg, g0 + gt, -1)
        out_norm[b] = np.where(fg, iou_pd[gi, np.arange(A)], 0.0)
        info.append(dict(n=n, near=int(near_box.sum()), skip=_skip_mask(n, A, gt, near_box, touched, cand), n_multi=int(multi.size), multi=multi,
                         multi_margin=mmargin, second=second, topk=dmargin, thr=tm))
    return torch.from_numpy(out_gt), torch.from_numpy(out_norm), info


def near_share(info):
    """(boxes of the case, boxes involved in a near-tied decision)"""
    return sum(i["n"] for i in info), sum(i["near"] for i in info)


def check_assignment(got_gt, got_norm, ref_gt, ref_norm, info):
    """-> (anchors whose assigned row differs, worst |got - ref| / (2^-16 |ref|) of the normalised metric, background values that are not exactly 0), all
    over the compared anchors."""
    skip = torch.from_numpy(np.stack([i["skip"] for i in info]))
    got_gt, got_norm = got_gt.detach().cpu().long(), got_norm.detach().cpu().double()
    cmp_ = ~skip
    wrong = int(((got_gt != ref_gt) & cmp_).sum())
    same_fg = cmp_ & (ref_gt >= 0) & (got_gt == ref_gt)
    rel = ((got_norm - ref_norm).abs() / (TAU * ref_norm.abs()).clamp_min(1e-300))[same_fg]
    bg = int(((got_norm != 0) & cmp_ & (ref_gt < 0)).sum())
    return wrong, (float(rel.max()) if rel.numel() else 0.0), bg


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# loss terms for a frozen assignment
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _giou_loss(b1, b2, eps=1e-10):
    x1, y1, x2, y2 = b1.unbind(-1); u1, v1, u2, v2 = b2.unbind(-1)
    inter = (torch.min(x2, u2) - torch.max(x1, u1)).clamp(0) * (torch.min(y2, v2) - torch.max(y1, v1)).clamp(0)
    union = (x2 - x1) * (y2 - y1 + eps) + (u2 - u1) * (v2 - v1 + eps) - inter + eps
    iou = inter / union
    c_area = (torch.max(x2, u2) - torch.min(x1, u1)) * (torch.max(y2, v2) - torch.min(y1, v1)) + eps
    return 1.0 - (iou - (c_area - union) / c_area)


def terms_ref(scores, distri, points, strides, gts, out_gt, out_norm, weights=(1.0, 2.5, 0.5), upstream=1.0, dtype=torch.float64, want_S=True):
    """scores [B,A,nc] in [0,1] and distri [B,A,68] logits (fp16 / fp32: upcast exactly), points [A,2], strides [A], gts [T,5], assignment out_gt [B,A]
    (row or -1) and out_norm [B,A]; weights = (class, iou, dfl) -> dict(out = (total, w_iou iou, w_dfl dfl, w_cls cls, target-score sum), gs, gd = the
    gradients of upstream * total, Ss, Sd = their sizes).  dtype = torch.float32 evaluates the same formulas in fp32 (for r32)."""
    wc, wi, wd = weights
    B, A, nc = scores.shape
    cpu = lambda t: t.detach().cpu()
    p = cpu(scores).to(dtype).requires_grad_(True)
    z = cpu(distri).to(dtype).view(B, A, 4, R1).requires_grad_(True)
    st = cpu(strides).to(dtype).reshape(A, 1)
    pts_s = cpu(points).to(dtype) / st
    g = cpu(gts).to(dtype)
    if g.shape[0] == 0:
        g = torch.zeros(1, 5, dtype=dtype)                                      # no labels: one all-zero row nobody is assigned to
    og = cpu(out_gt).long()
    fg = og >= 0
    idx = og.clamp(min=0)
    t = cpu(out_norm).to(dtype) * fg
    labels = g[:, 0].long()[idx]
    one_hot = F.one_hot(torch.where(fg, labels, torch.full_like(labels, nc)), nc + 1)[..., :-1].to(dtype)
    t_scores = one_hot * t.unsqueeze(-1)
    w = 0.75 * p.pow(2.0) * (1 - one_hot) + t_scores * one_hot                  # loss.py:196-206: the gradient flows through the weight too
    tss = t_scores.sum()
    cls = (F.binary_cross_entropy(p, t_scores, reduction="none") * w).sum() / tss
    t_boxes = g[:, 1:][idx] * fg.unsqueeze(-1) / st                              # loss.py:152
    raw = torch.cat([pts_s - t_boxes[..., :2], t_boxes[..., 2:] - pts_s], -1)
    ltrb = raw.clip(0, R1 - 1 - 0.01)
    clips = (int((raw[fg] < 0).sum()), int((raw[fg] > R1 - 1 - 0.01).sum()))       # DFL targets clipped at 0 / at 15.99
    tl = ltrb.long()
    wl = (tl + 1).to(dtype) - ltrb
    if float(tss) > 0:
        dist = F.softmax(z, -1).matmul(torch.arange(R1, dtype=dtype))
        pb = torch.cat([pts_s - dist[..., :2], pts_s + dist[..., 2:]], -1)
        iou = (_giou_loss(pb, t_boxes) * t)[fg].sum() / tss
        logp = F.log_softmax(z, -1)
        ce = -(logp.gather(-1, tl.unsqueeze(-1)).squeeze(-1) * wl + logp.gather(-1, (tl + 1).unsqueeze(-1)).squeeze(-1) * (1 - wl))
        dfl = (ce.mean(-1) * t)[fg].sum() / tss
    else:                                                                            # no foreground: BboxLoss returns zeros (loss.py:262-266)
        iou = dfl = torch.zeros((), dtype=dtype)
    total = wc * cls + wi * iou + wd * dfl
    gs, gd = torch.autograd.grad(total * upstream, [p, z], allow_unused=True)
    gd = torch.zeros_like(z) if gd is None else gd
    res = dict(out=torch.stack([total, wi * iou, wd * dfl, wc * cls, tss]).detach().double(), gs=gs.double(), gd=gd.reshape(B, A, 4 * R1).double(), fg=fg, clips=clips)
    res["kink"] = torch.zeros_like(fg)
    if not want_S:
        return res
    # ---- sizes: every term of the gradient in absolute value, in fp64
    with torch.no_grad():
        p, z = p.detach().double(), z.detach().double()
        sc = abs(upstream) * wc / tss.double()
        den = (p * (1 - p)).clamp_min(1e-12)
        l1 = torch.log(1 - p).clamp_min(-100.0)
        Ss = sc * (2 * 0.75 * p ** 3 / den + 1.5 * p * (l1.abs() + 1.0))           # negatives: 0.75 p^3 / (p (1 - p)) - 1.5 p log(1 - p)
        td = t.double()
        pk = p.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
        Sp = sc * td * 2 * (pk + td) / (pk * (1 - pk)).clamp_min(1e-12)            # positives: t (p - t) / (p (1 - p))
        Ss = torch.where(one_hot > 0, Sp.unsqueeze(-1).expand_as(Ss), Ss)
        Sd = torch.zeros_like(z)
        if float(tss) > 0:
            up = abs(upstream) / tss.double()
            m = z.max(-1, keepdim=True)[0]
            q = F.softmax(z, -1)
            qa = q * (1 + (z - m).abs())
            ks = torch.arange(R1, dtype=torch.float64)
            D = (qa * ks).sum(-1)                                                  # [B,A,4]
            d = (q * ks).sum(-1)
            ps, ss = pts_s.double(), st.double()
            x1, y1, x2, y2 = ps[:, 0] - d[..., 0], ps[:, 1] - d[..., 1], ps[:, 0] + d[..., 2], ps[:, 1] + d[..., 3]
            tb = g.double()[:, 1:][idx] * fg.unsqueeze(-1) / ss
            u1, v1, u2, v2 = tb.unbind(-1)
            e = 1e-10
            w1, h1, w2, h2 = x2 - x1, y2 - y1 + e, u2 - u1, v2 - v1 + e
            iw = (torch.min(x2, u2) - torch.max(x1, u1)).clamp(0); ih = (torch.min(y2, v2) - torch.max(y1, v1)).clamp(0)
            inter = iw * ih
            uni = w1 * h1 + w2 * h2 - inter + e
            cw = torch.max(x2, u2) - torch.min(x1, u1); ch = torch.max(y2, v2) - torch.min(y1, v1)
            car = cw * ch + e
            # kinks: autograd (and the kernel) take one-sided derivatives of min / max / clamp; where a predicted coordinate lies within tau of the target's,
            # or the overlap within tau of 0, fp32 and fp64 may stand on different sides and the GIoU gradient jumps.  Such anchors are near-tied decisions
            # like those of the assigner: their distri rows are left out (exact equality is the 0.5 / 0.5 sub-gradient on both sides and is compared).
            # The overlap of a predicted box that lies inside the target along an axis is its own extent d_left + d_right >= 0, whatever its size: no kink.
            near0 = lambda v, sc_: (v != 0) & (v.abs() < TAU * sc_)
            sx = torch.max(torch.max(u1.abs(), u2.abs()), ps[:, 0].abs().expand_as(u1)).clamp_min(1.0)
            sy = torch.max(torch.max(v1.abs(), v2.abs()), ps[:, 1].abs().expand_as(v1)).clamp_min(1.0)
            own_x, own_y = (x2 <= u2) & (x1 >= u1), (y2 <= v2) & (y1 >= v1)
            kink = fg & (near0(x1 - u1, sx) | near0(x2 - u2, sx) | near0(y1 - v1, sy) | near0(y2 - v2, sy)
                         | (~own_x & near0(torch.min(x2, u2) - torch.max(x1, u1), sx)) | (~own_y & near0(torch.min(y2, v2) - torch.max(y1, v1), sy)))
            res["kink"] = kink
            Sdd = []
            for side in range(4):
                xs = side % 2 == 0
                dinter = ih if xs else iw
                darea = h1.abs() if xs else w1.abs()
                duni = darea + dinter
                dcar = ch if xs else cw
                Sdd.append((dinter * uni.abs() + inter * duni) / uni ** 2 + (duni * car + uni.abs() * dcar) / car ** 2)
            Sdd = torch.stack(Sdd, -1)                                             # [B,A,4]
            # the two target weights wl = (tl + 1) - tgt, wr = 1 - wl with their terms in absolute value: tgt = px - u is rounded once in fp32
            wa = ((tl + 1).double() + ltrb.double()).unsqueeze(-1)
            wl_k = F.one_hot(tl, R1).double() * wa + F.one_hot(tl + 1, R1).double() * (1 + wa)
            Sd = (up * td).unsqueeze(-1).unsqueeze(-1) * (wi * Sdd.unsqueeze(-1) * qa * (ks + D.unsqueeze(-1)) + 0.25 * wd * (qa + wl_k))
            Sd = Sd * fg.unsqueeze(-1).unsqueeze(-1)
        res["Ss"], res["Sd"] = Ss, Sd.reshape(B, A, 4 * R1)
    return res


def grad_ratio(got, ref, S, dtype, k=K):
    """|got - ref| / (ulp_T(ref) + k 2^-24 S) per element.  Where the fp64 value is not finite or overflows `dtype` the same infinity (or NaN: 0 * inf
    when the target-score sum is 0) is required: ratio 0 if it is there, inf if not."""
    got = got.detach().cpu().double()
    big = torch.finfo(dtype).max
    over = ~torch.isfinite(ref) | (ref.abs() > big) | ~torch.isfinite(S)
    refc = torch.where(over, torch.zeros_like(ref), ref)
    r = (torch.where(over, torch.zeros_like(got), got) - refc).abs() / (ulp(refc, dtype) + k * 2.0 ** -24 * torch.where(over, torch.zeros_like(S), S))
    same = torch.where(torch.isnan(ref), torch.isnan(got), torch.isinf(got) & (torch.sign(got) == torch.sign(ref)))
    near_max = torch.isfinite(ref) & (ref.abs() <= big * (1 + 2.0 ** -10)) & (got.abs() >= big)       # rounds either side of the largest finite value
    return torch.where(over, torch.where(same | near_max, torch.zeros_like(r), torch.full_like(r, math.inf)), r)


def distri_ratio(got, res, dtype, k=K):
    """grad_ratio of the distri gradient with the rows of kink anchors left out -> (worst ratio, background rows that are not exactly 0, kink anchors)"""
    B, A = res["fg"].shape
    r = grad_ratio(got, res["gd"], res["Sd"], dtype, k).view(B, A, -1)
    r = torch.where(res["kink"].unsqueeze(-1), torch.zeros_like(r), r)
    bad_bg = int((got.detach().cpu().view(B, A, -1)[~res["fg"]] != 0).any(-1).sum())
    return float(r.max()), bad_bg, int(res["kink"].sum())


def check_sums(got, ref, rel=5e-5):
    """the five sums: relative 5e-5, the same infinities -> worst |got - ref| / (rel |ref|)"""
    got = got.detach().cpu().double()
    worst = 0.0
    for a, b in zip(got.tolist(), ref.tolist()):
        if not math.isfinite(b):
            worst = max(worst, 0.0 if (a == b or (math.isnan(a) and math.isnan(b))) else math.inf)
        else:
            worst = max(worst, abs(a - b) / (rel * abs(b)) if b != 0 else (0.0 if a == 0 else math.inf))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# cases (shared by tests/test_gpu_loss_edges.py and tests/test_loss_ref_host.py)
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _class_cycle(nc):
    """class 0, class nc - 1, then one class in each of the 8 lanes of loss_cls_kernel's 8-wide vectors (9 j mod nc, j = 1..7)"""
    return [0, nc - 1] + [(9 * j) % nc for j in range(1, 8)]


def terms_case(nc, dtype, size, B, seed=0):
    """Synthetic frozen assignment for the loss-term kernels.  -> dict(name, size, hw, scores, distri [dtype], targets [T,6] grouped by image, out_gt [B,A]
    int32 rows of the grouped targets, out_norm [B,A] fp32, forced = flat indices of the planted foreground anchors, empty_tile)."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * nc + (1 if dtype == torch.float16 else 0) + size + 31 * B)
    hw = [(size // s, size // s) for s in (8, 16, 32)]
    pts, st = anchors(hw, (8, 16, 32))
    A = pts.shape[0]
    NA = B * A
    cyc = _class_cycle(nc)
    rows = []
    for b in range(B):
        # row 0: the whole image; row 1: a small box in the top-left corner that most anchors lie outside of (the DFL target clips at 0 on the sides facing
        # it); row 2: a box five times the image (clips at 15.99 from every anchor, at any image size; its coordinates are exact in fp32)
        rows.append([b, cyc[0], 0.5, 0.5, 1.0, 1.0])
        rows.append([b, cyc[1], 0.07, 0.09, 0.11, 0.13])
        rows.append([b, cyc[2], 0.5, 0.5, 5.0, 5.0])
        for j in range(3, 11):
            wh = torch.rand(2, generator=g) * 0.5 + 0.08
            c = torch.rand(2, generator=g)
            rows.append([b, cyc[j % len(cyc)], float(c[0]), float(c[1]), float(wh[0]), float(wh[1])])
    targets = torch.tensor(rows, dtype=torch.float32)
    targets[:, 2:] = torch.round(targets[:, 2:] * 4096) / 4096                  # a 2^-12 lattice: the fp32 label preprocessing is exact (see host_gts)
    per = 11
    scores = torch.sigmoid(torch.randn(B, A, nc, generator=g) * 1.5 - 2.0)
    big = 20.0 if dtype == torch.float16 else 30.0
    distri = torch.randn(B, A, 4 * R1, generator=g) * 1.2
    fgm = torch.rand(NA, generator=g) < (0.3 if NA < 1000 else 0.12)
    forced = sorted({0, NA - 1, 63, 64, min(127, NA - 1)} | {b * A for b in range(B)} | {b * A + A - 1 for b in range(B)})
    tiles = (NA + 63) // 64
    free = [t_ for t_ in range(tiles) if not any(t_ * 64 <= f < t_ * 64 + 64 for f in forced)]
    empty_tile = free[len(free) // 2] if free else -1
    fgm[16:32] = False                                                           # a wave (16 anchors x 4 sides) of the first tile with no foreground
    if empty_tile >= 0:
        fgm[empty_tile * 64:empty_tile * 64 + 64] = False
    fgm[forced] = True
    flat = torch.nonzero(fgm).reshape(-1)
    nf = flat.numel()
    img = flat // A
    row = torch.randint(0, per, (nf,), generator=g)
    row[::4] = 0                                                                 # every fourth foreground anchor: the whole-image box
    row[2::4] = 1                                                                # two on: the corner box it (mostly) lies outside of
    row[1::2] = 2 + torch.arange(row[1::2].numel()) % 9                          # between them the class cycle, so every lane has a positive class
    out_gt = torch.full((NA,), -1, dtype=torch.int32)
    out_gt[flat] = (img * per + row).int()
    norm = torch.rand(nf, generator=g) * 0.95 + 0.05
    norm[0::7] = 1.0
    norm[3::7] = 2.0 ** -20
    out_norm = torch.zeros(NA)
    out_norm[flat] = norm
    # planted scores: exact 0, exact 1 (fp16 saturation), 2^-24, 1 - 2^-11 — on negatives everywhere, and on the positive class of some foreground anchors
    special = torch.tensor([0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -11])
    sflat = scores.view(NA, nc)
    neg_a = torch.randint(0, NA, (64,), generator=g)
    neg_c = torch.randint(0, nc, (64,), generator=g)
    sflat[neg_a, neg_c] = special[torch.arange(64) % 4]
    lab_fg = targets[:, 1].long()[out_gt[flat].long()]
    pick = torch.arange(0, nf, 3)
    sflat[flat[pick], lab_fg[pick]] = special[torch.arange(pick.numel()) % 4]
    # planted distri rows: all mass on bin 0 (zero-size predicted box), all on bin 16, +-big; on foreground anchors (background rows are never read)
    dflat = distri.view(NA, 4, R1)
    for j, a in enumerate(flat[1::4].tolist()):
        kind = j % 3
        if kind == 0:
            dflat[a] = 0.0; dflat[a, :, 0] = big
        elif kind == 1:
            dflat[a] = 0.0; dflat[a, :, 16] = big
        else:
            dflat[a] = (torch.randint(0, 2, (4, R1), generator=g).float() * 2 - 1) * big
    scores = scores.to(dtype)
    distri = distri.to(dtype)
    name = "terms_nc%d_%s_B%d_%d" % (nc, "f16" if dtype == torch.float16 else "f32", B, size)
    return dict(name=name, size=size, hw=hw, nc=nc, scores=scores, distri=distri, targets=targets, out_gt=out_gt.view(B, A), out_norm=out_norm.view(B, A),
                forced=forced, empty_tile=empty_tile, points=pts, strides=st)


TERMS_NC = (1, 3, 8, 20, 80, 81)


def _kinds(b, cyc, atss):
    """the box kinds every assigner case holds (image b): zero width, thinner than a cell, wholly outside the image, the whole image, partly outside, an exact
    duplicate, nested boxes with one centre; ATSS: an all-zero row, a centre in each corner cell, a centre exactly on a cell corner"""
    c = lambda j: cyc[j % len(cyc)]
    # coordinates with many digits: "nice" decimals put centres a whole number of tenths of a cell from the anchors and make sums of squares coincide up to
    # rounding (near-ties of the ATSS distances); the one box that is meant to tie is dyadic, so its ties are exact in fp32 and fp64 alike
    rows = [[b, c(0), 0.4031, 0.4517, 0.0, 0.3029],                                # zero width
            [b, c(1), 0.6137, 0.3719, 0.0041, 0.4523],                             # thinner than a stride-8 cell at every size used
            [b, c(2), 1.1513, 1.1537, 0.2011, 0.2039],                             # wholly outside (within the binade of the image size)
            [b, c(3), 0.5, 0.5, 1.0, 1.0],                                         # the whole image
            [b, c(4), 0.9307, 0.1213, 0.4031, 0.5051],                             # partly outside
            [b, c(5), 0.3147, 0.6791, 0.2617, 0.3433], [b, c(5), 0.3147, 0.6791, 0.2617, 0.3433],      # exact duplicates
            [b, c(6), 0.6619, 0.6311, 0.5227, 0.4813], [b, c(7), 0.6619, 0.6311, 0.2719, 0.2207]]      # nested, same centre
    if atss:
        rows += [[b, c(8), 0.0, 0.0, 0.0, 0.0],                                    # all-zero row (mask_gt)
                 [b, c(0), 0.0313, 0.0419, 0.0523, 0.0711], [b, c(1), 0.9701, 0.0317, 0.0509, 0.0521], [b, c(2), 0.0211, 0.9803, 0.0307, 0.0311],
                 [b, c(3), 0.9807, 0.9709, 0.0303, 0.0517],                        # a centre in each corner cell: the 9 x 9 window is clamped
                 [b, c(4), 0.5, 0.5, 0.25, 0.25]]                                  # centre on a cell corner of every level, fp32-exact: exact distance ties
    return rows


def _random_rows(g, b, n, nc, lo=0.05, hi=0.45):
    out = []
    for _ in range(n):
        wh = torch.rand(2, generator=g) * (hi - lo) + lo
        c = torch.rand(2, generator=g)
        out.append([b, int(torch.randint(0, nc, (1,), generator=g)), float(c[0]), float(c[1]), float(wh[0]), float(wh[1])])
    return out


#            name                 atss   size  level_hw                        strides          nc  dtype           B  (alpha, beta) random boxes per image, seed
_ASSIGN = [("tal_64_nc1",        False, 64,  None,                           (8, 16, 32),     1,  torch.float32,  2, (1.0, 6.0),   [3, 0],   1),
           ("tal_96_nc3_f16",    False, 96,  None,                           (8, 16, 32),     3,  torch.float16,  2, (0.5, 2.5),   [4, 9],   2),
           ("tal_320_f16_zero",  False, 320, None,                           (8, 16, 32),     80, torch.float16,  2, (1.0, 6.0),   [12, 25], 3),
           ("tal_320_a2b2",      False, 320, None,                           (8, 16, 32),     3,  torch.float32,  1, (2.0, 2.0),   [20],     4),
           ("tal_nonsquare",     False, 96,  [(5, 12), (3, 6), (2, 3)],      (8, 16, 32),     3,  torch.float32,  2, (1.0, 6.0),   [3, 5],   5),
           ("tal_1level_A60",    False, 96,  [(5, 12)],                      (8,),            80, torch.float16,  2, (1.0, 6.0),   [3, 2],   6),
           ("tal_4levels",       False, 320, [(40, 40), (20, 20), (10, 10), (5, 5)], (8, 16, 32, 64), 1, torch.float32, 1, (0.5, 2.5), [15], 7),
           ("tal_T1500",         False, 320, None,                           (8, 16, 32),     80, torch.float32,  4, (1.0, 6.0),   None,     8),
           ("tal_640_crowd",     False, 640, None,                           (8, 16, 32),     80, torch.float32,  2, (1.0, 6.0),   None,     9),
           ("atss_96_nc3",       True,  96,  None,                           (8, 16, 32),     3,  torch.float32,  2, None,         [4, 0],   11),
           ("atss_320",          True,  320, None,                           (8, 16, 32),     80, torch.float16,  2, None,         [12, 25], 12),
           ("atss_nonsquare",    True,  96,  [(5, 12), (3, 6), (3, 3)],      (8, 16, 32),     1,  torch.float32,  2, None,         [3, 5],   13),
           ("atss_ungrouped",    True,  320, None,                           (8, 16, 32),     20, torch.float32,  3, None,         [5, 0, 7], 15)]
ASSIGN_NAMES = [c[0] for c in _ASSIGN]
F16_DISTRI = ("tal_96_nc3_f16", "tal_1level_A60", "atss_nonsquare")   # fp16 logits: loss_decode_kernel<_Float16>; A = 189, 60, 87: a partial last tile of 64 anchors
ZERO_FILL = ("tal_320_f16_zero", "tal_1level_A60")                     # cases that must reach the zero-metric fill through scores that are exactly 0


def assign_case(name):
    """-> dict(name, atss, size, hw, strides, nc, B, alpha, beta, scores [dtype], distri fp32, targets [T,6], points, stride per anchor)"""
    _, atss, size, hw, strides, nc, dtype, B, ab, nrand, seed = [c for c in _ASSIGN if c[0] == name][0]
    g = torch.Generator().manual_seed(5000 + seed)
    hw = hw or [(size // s, size // s) for s in strides]
    pts, st = anchors(hw, strides)
    A = pts.shape[0]
    cyc = _class_cycle(nc)
    scores = torch.sigmoid(torch.randn(B, A, nc, generator=g) * 1.5 - 2.0)
    distri = torch.randn(B, A, 4 * R1, generator=g) * 1.2
    if name == "tal_T1500":
        # 1500 ungrouped labels over 4 images (more rows than threads of tal_targets_kernel), 60 of them with image ids -1, B and B + 3 that must vanish
        rows = []
        for i in range(1500):
            b = int(torch.randint(0, B, (1,), generator=g))
            rows += _random_rows(g, b, 1, nc, 0.02, 0.2)
        for i in range(0, 1500, 25):
            rows[i][0] = (-1, B, B + 3)[(i // 25) % 3]
        for r in rows:                                                            # a 2^-12 lattice: the fp32 preprocessing is exact there (see host_gts); this
            r[2:] = [round(v * 4096) / 4096 for v in r[2:]]                       # case is about row order, offsets and dropped rows
    elif name == "tal_640_crowd":
        # image 0: 600 small disjoint boxes on a 30 x 20 lattice, the whole list twice (rows j and j + 600 are equal): 1200 > kGtL boxes, and every anchor a
        # box picks is claimed by its duplicate too: > kMulti multiply-claimed anchors; equal IoU -> the first row.  image 1: 3 boxes.
        one = []
        for j in range(600):
            ix, iy = j % 30, j // 30
            one.append([0, int(torch.randint(0, nc, (1,), generator=g)), (ix + 0.5) / 30, (iy + 0.5) / 20, 0.97 / 30, 0.97 / 20])
        rows = one + [list(r) for r in one] + _random_rows(g, 1, 3, nc)
    else:
        rows = []
        for b in range(B):
            rows += _kinds(b, cyc, atss) + _random_rows(g, b, nrand[b], nc)
    if name == "atss_ungrouped":
        # labels in any order, with rows of images -1, B and B + 3 that must vanish (the guard of atss_cand_kernel, tal_assign.hip:308)
        rows += [[-1, 1, 0.31, 0.42, 0.2, 0.2], [B, 2, 0.52, 0.43, 0.3, 0.2], [B + 3, 3, 0.63, 0.54, 0.2, 0.3]]
        rows = [rows[i] for i in torch.randperm(len(rows), generator=g).tolist()]
    targets = torch.tensor(rows, dtype=torch.float32)
    if "zero" in name or name == "tal_1level_A60":
        # scores that are exactly 0 on the class of a box inside it (fp16 underflow): the zero-metric fill decides among anchors that lie inside.  The box
        # covers the first anchors of level 0, where the fill looks (zeros are taken in anchor order from anchor 0).  Only the last few inside anchors keep a
        # positive score: fewer than 13 positive metrics, so the other picks are zero-score anchors 0, 1, ... of which those in the first row lie inside.
        extra = torch.tensor([[0, cyc[2], 0.12, 0.15, 0.22, 0.28]], dtype=torch.float32)
        targets = torch.cat([extra, targets])
        inside = torch.nonzero((pts[:, 0] > 0.01 * size) & (pts[:, 0] < 0.23 * size) & (pts[:, 1] > 0.01 * size) & (pts[:, 1] < 0.29 * size)).reshape(-1)
        zero = inside[:-min(5, inside.numel() // 3)]
        scores[0, zero, cyc[2]] = 0.0
        scores[0, inside[-min(5, inside.numel() // 3):], cyc[2]] = 0.5
    if dtype == torch.float16:
        scores = (scores - 6e-8).clamp_min(0).half()                             # round to fp16: tiny scores underflow to exact 0 on their own as well
    if name in F16_DISTRI:
        distri = distri.half()
    a, bt = ab if ab else (1.0, 1.0)
    return dict(name=name, atss=atss, size=size, hw=hw, strides=strides, nc=nc, B=B, alpha=a, beta=bt, scores=scores, distri=distri, targets=targets,
                points=pts, stride=st)


def assign_ref(case, gts, offs, boxes):
    """the fp64 assignment of a case on the given (device- or host-made) preprocessed rows and decoded boxes"""
    if case["atss"]:
        return atss_ref(anchor_boxes(case["points"], case["stride"]), [h * w for h, w in case["hw"]], boxes, gts, offs, 9)
    return tal_ref(case["scores"], boxes, case["points"], gts, offs, case["nc"], 13, case["alpha"], case["beta"], 1e-9)


def host_inputs(case):
    """the fp32 stand-ins of the device preprocessing and decode (for the near-tie census and the fp32-oracle comparison on a machine without a GPU)"""
    t = case["targets"]
    B, size = case["B"], float(case["size"])
    _, im, offs, keep = targets_ref(t, B, size)
    r = t[keep]
    xy, wh = r[:, 2:4] * size, r[:, 4:6] * size
    gts = torch.cat([r[:, 1:2], xy - wh / 2, xy + wh / 2], 1)
    return gts, offs, decode_f32(case["distri"], case["points"], case["stride"])


def host_gts(targets, B, size):
    """fp32 stand-in of tal_targets_kernel (the reference's own fp32 sequence: scale, then xywh -> xyxy) -> (rows [n,5] fp32, offsets).  Three roundings: up
    to 1.25 ulp of the image size from the fp64 rows in the worst case, and about one coordinate in 2000 of random labels is past 1 ulp.  check_targets asks
    for 1 ulp, so the cases are chosen (fixed coordinates, seeds) such that this plain fp32 sequence is within it: tests/test_loss_ref_host.py asserts that
    for every case, from the reference and fp32 arithmetic alone."""
    _, im, offs, keep = targets_ref(targets, B, float(size))
    r = targets[keep].float()
    xy, wh = r[:, 2:4] * float(size), r[:, 4:6] * float(size)
    return torch.cat([r[:, 1:2], xy - wh / 2, xy + wh / 2], 1), offs


def terms_cases():
    """every synthetic loss-term case of tests/test_gpu_loss_edges.py: (nc, dtype, size, B)"""
    out = [(nc, dt, 64, B) for nc in TERMS_NC for dt in (torch.float32, torch.float16) for B in (1, 3)]
    return out + [(80, torch.float32, 320, 32), (80, torch.float16, 320, 32)]


def background_case(dtype):
    """no foreground anchor at all: cls is inf, the box terms and the box gradient are 0"""
    c = terms_case(80, dtype, 64, 3, seed=5)
    c["out_gt"] = torch.full_like(c["out_gt"], -1)
    c["out_norm"] = torch.zeros_like(c["out_norm"])
    c["name"] = "background_" + ("f16" if dtype == torch.float16 else "f32")
    return c
