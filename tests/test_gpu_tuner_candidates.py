"""-m gpu: every launch variant the autotuner can pick (tuner.candidates), run at the shapes where the benchmarked plans run it, against the fp64
restatement of its op (tests/op_ref.py) with a per-element bound — and the frozen tables bench.py loads (profiles/round6_tune*.json) built into plans.

The plans are walked op by op on one stream (Plan.launch_op): before op i runs, its sources are snapshot from the arena; every candidate of op i
(deduplicated by tuner signature across plans) writes to a scratch buffer that holds NaN in the op's slice and a sentinel elsewhere; the slice must
meet the bound, the rest must keep the sentinel.  Then the plan's own configuration of op i runs into the arena and the walk goes on.  A depth-wise
op's list is taken with the 1x1 conv in front of it at tile_k = 5 where the tuner may put it there, so the pixel-pair variants are in it; they read a
genuine pair-layout copy of their input.  Stem pairs and head tails (no fp64 restatement here) must reproduce the plan's own configuration."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import maf_yolo_amd as M
from maf_yolo_amd import engine, lib, pack, train_ops, tuner
from oracle import maf_oracle as O
import op_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = 1234.0
_KIND = {lib.OP_CONV1X1: "conv1x1", lib.OP_CONV3X3S2: "conv3x3s2", lib.OP_DWCONV: "dwconv", lib.OP_STEM2: "stem2", lib.OP_BOTTLENECK: "bottleneck",
         lib.OP_CONV1DW: "conv1dw", lib.OP_SPPF_POOL: "sppf pool", lib.OP_HEADTAIL: "headtail"}
_TK = lib.CONV_VARIANT_NAMES


def _launch(op):
    lib.check(lib.load().maf_op_launch(C.byref(op), torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize(DEV)


def _family(kind, tiles, pairs_out=False):
    tp, tc, tk = tiles
    if kind in (lib.OP_CONV1X1, lib.OP_CONV3X3S2):
        name = "conv1x1" if kind == lib.OP_CONV1X1 else "conv3x3s2"
        return "%s tile_k=%d %s%s%s" % (name, tk, _TK[tk], " w8" if tk == 5 and tp == 2 else "", " pairs-out" if pairs_out else "")
    if kind == lib.OP_DWCONV:
        return {-1: "dw matrix-core", -2: "dw dot2"}.get(tp, "dw pixel-pair staged" if tp == -4 and tk & 128 else "dw pixel-pair" if tp == -4 else "dw generic")
    if kind == lib.OP_STEM2:
        return "stem2 rows=%d" % tp
    return "headtail iters=%d" % tk


def _model(scale, fuse=None):
    m = M.Model(scale)
    m.load_state_dict(O.synth_state_dict(scale, 0))
    m = m.to(DEV).eval()
    m.autotune = True                    # (the plan form of tuned plans: MPRep in one launch where it exists; no timing happens here)
    if fuse is not None:
        m.fuse_bottlenecks = fuse
    return m


def _plan(m, B, H, W):
    with torch.no_grad():
        return engine.Plan(m, B, H, W, lib.F16, lib.F16, DEV)


def _slice(plan, seg):
    return plan.view(seg.buf)[..., seg.coff:seg.coff + seg.C].clone()


def _scratch(buf, B, f32, slices, pairs=False):
    t = torch.full((B, buf.H, buf.W, buf.stride), SENT, dtype=torch.float32 if f32 else torch.float16, device=DEV)
    for lo, hi in slices:
        t[..., lo:hi] = float("nan")
    if pairs:
        t = pack.pairs_from_nhwc(t)
    return t


def _nhwc(t):
    """Back from the pixel-pair layout [B, H, W/2, C, 2]."""
    b, h, w2, c, _ = t.shape
    return t.transpose(3, 4).reshape(b, h, 2 * w2, c)


def _check(got, ref, bnd, S, what):
    """got: the output slice; returns max |got - ref| / bound."""
    assert torch.isfinite(got).all(), "%s: non-finite (unwritten) outputs" % what
    q = (got.double() - ref).abs() / bnd
    r = q.max().item()
    if r > 1:
        idx = np.unravel_index(int(q.argmax()), tuple(ref.shape))
        raise AssertionError("%s: |got - ref| / bound = %.3g at %s (got %.6g, ref %.6g, bound %.4g)" % (what, r, idx, got[idx].item(), ref[idx].item(), bnd[idx].item()))
    return r


def _width(op):
    return op.nc if op.kind == lib.OP_BOTTLENECK and op.nc else op.Cout // 2 if op.kind == lib.OP_STEM2 and op.aux[0] else op.Cout


def _run(plan, i, op, refs, x, pairs_out=False):
    """Launch `op` (a variant of op i, or its plan configuration) into scratch buffers, check each output against `refs` and that nothing outside the
    op's slices changed; returns the worst |got - ref| / bound."""
    rec = plan._ops[i]
    B = plan.B
    what = "%s %s" % (plan.op_names[i], (op.tile_p, op.tile_c, op.tile_k))
    if op.kind == lib.OP_HEADTAIL:
        sc = torch.full((B, plan.A, 5 + plan.nc), float("nan"), device=DEV)
        op.out = sc.data_ptr()
        _launch(op)
        lo, hi = op.Hin, op.Hin + op.H * op.W
        worst = _check(sc[:, lo:hi], *refs["out"], what)
        assert sc[:, :lo].isnan().all() and sc[:, hi:].isnan().all(), "%s wrote outside its rows" % what
        return worst
    if op.kind == lib.OP_STEM2:
        op.src[0].ptr = x.data_ptr()
    w = _width(op)
    slices = [(op.out_coff, op.out_coff + w)] + ([(0, rec["pool1"][0].shape[0])] if rec.get("pool1") else [])
    sc = _scratch(rec["out"], B, op.out_f32, slices, pairs_out)
    op.out = sc.data_ptr()
    op.out_pairs = int(pairs_out)
    extra = []                                                           # (name in refs, scratch, channels)
    if rec.get("twin"):
        extra.append(("twin", _scratch(rec["twin"]["out"], B, False, [(0, op.Cout)]), op.Cout))
        op.aux[3] = extra[-1][1].data_ptr()
    if op.kind == lib.OP_STEM2 and op.aux[0]:
        extra.append(("out2", _scratch(rec["out2"], B, False, [(0, w)]), w))
        op.aux[0] = extra[-1][1].data_ptr()
    _launch(op)
    got = _nhwc(sc) if pairs_out else sc
    worst = _check(got[..., op.out_coff:op.out_coff + w], *refs["out"], what)
    if "pool" in refs:
        worst = max(worst, _check(got[..., :slices[1][1]], *refs["pool"], what + " pooled branch"))
    for lo, hi in slices:
        got[..., lo:hi] = SENT
    assert (got == SENT).all(), "%s wrote outside its slice" % what
    for name, t, c in extra:
        worst = max(worst, _check(t[..., :c], *refs[name], what + " " + name))
        t[..., :c] = SENT
        assert (t == SENT).all(), "%s: %s written outside its slice" % (what, name)
    return worst


def _dw_tiles_with_pairs(plan, i):
    """The depth-wise op's candidates as the tuner offers them with the conv in front at tile_k = 5 where it may pick that (else as the plan stands)."""
    p = plan.ops[i - 1] if i > 0 else None
    if p is not None and p.kind == lib.OP_CONV1X1 and any(t[2] == 5 for t in tuner.conv_tiles(plan, i - 1)):
        keep = p.tile_k
        p.tile_k = 5
        try:
            return tuner.candidates(plan, i)
        finally:
            p.tile_k = keep
    return tuner.candidates(plan, i)


def walk(plan, x, seen, stats, worst, mutate=None):
    """Walk `plan` op by op (see the module docstring).  seen: (signature, tiles, pairs-out) already run; stats: family -> count; worst: family (or op kind
    in its plan configuration) -> max |got - ref| / bound.  Returns (candidates enumerated, launched, skipped as already run, pred)."""
    B = plan.B
    pred = torch.full((B, plan.A, 5 + plan.nc), float("nan"), device=DEV)
    enumerated = launched = dup = 0
    for i, (o, rec) in enumerate(zip(plan.ops, plan._ops)):
        kind = o.kind
        if kind != lib.OP_DECODE:
            sig = tuner.signature(plan, i)
            srcs = [_slice(plan, s) for s in rec["segs"]]
            twin_src = _slice(plan, rec["twin"]["seg"]) if rec.get("twin") else None
            refs = op_ref.reference(o, rec, srcs, DEV, twin_src, image=x)
            cands = _dw_tiles_with_pairs(plan, i) if kind == lib.OP_DWCONV else tuner.candidates(plan, i)
            jobs = [(c_, False) for c_ in cands]
            if kind == lib.OP_CONV1X1 and sig[-1] == "pairs":         # the pair epilogue of the LDS-weight kernel, as a plan with a pair-reading consumer runs it
                jobs += [(c_, True) for c_ in cands if c_.tiles[2] == 5]
            enumerated += len(jobs)
            for c_, pairs_out in jobs:
                key = (sig, c_.tiles, pairs_out)
                if key in seen:
                    dup += 1
                    continue
                if mutate is not None and not mutate(plan, i, c_):
                    continue
                op = c_.op
                pin = None
                if c_.pairs:                                           # a genuine pair-layout copy of the whole input buffer
                    pin = pack.pairs_from_nhwc(plan.view(rec["segs"][0].buf).contiguous())
                    op.src[0].ptr = pin.data_ptr()
                fam = _family(kind, c_.tiles, pairs_out)
                r = _run(plan, i, op, refs, x, pairs_out)
                seen.add(key)
                stats[fam] = stats.get(fam, 0) + 1
                worst[fam] = max(worst.get(fam, 0.0), r)
                launched += 1
                del pin
            if mutate is None:                                       # the plan's own configuration, tuned kind or not: same bound
                r = _run(plan, i, lib.MafOp.from_buffer_copy(o), refs, x)
                fam = "plan config: " + _KIND[kind]
                worst[fam] = max(worst.get(fam, 0.0), r)
                stats[fam] = stats.get(fam, 0) + 1
        plan.launch_op(i, image_ptr=x.data_ptr(), pred_ptr=pred.data_ptr())
        torch.cuda.synchronize(DEV)
    return enumerated, launched, dup, pred


# (scale, batch, H, W, fuse_bottlenecks): the headline, the two other bench legs, the latency leg (split-K and the small-M filters), an 11 x 19 P5
# level (odd W: no pixel pairs, ragged tiles), and the headline with fuse_bottlenecks True / 2 / False: their new tuned signatures are few (the
# walk skips what it has run), but their BOTTLENECK (fused everywhere), CONV1DW and unfused-chain ops are checked at the bench shape in plan configuration
PLANS = [("n", 32, 640, 640, None), ("s", 32, 640, 640, None), ("m", 32, 640, 640, None), ("m", 1, 640, 640, None), ("n", 3, 352, 608, None),
         ("n", 32, 640, 640, True), ("n", 32, 640, 640, 2), ("n", 32, 640, 640, False)]


def test_every_candidate_of_every_op_meets_the_fp64_bound():
    seen, stats, worst = set(), {}, {}
    t0 = time.time()
    total_e = total_l = 0
    kinds = set()
    for scale, B, H, W, fuse in PLANS:
        m = _model(scale, fuse)
        plan = _plan(m, B, H, W)
        x = O.synth_images(B, (H, W), seed=5).to(DEV).half()
        expected = sum(len(_dw_tiles_with_pairs(plan, i) if o.kind == lib.OP_DWCONV else tuner.candidates(plan, i)) for i, o in enumerate(plan.ops))
        e, launched, dup, pred = walk(plan, x, seen, stats, worst)
        assert e >= expected and launched + dup == e, (scale, B, H, W, fuse, expected, e, launched, dup)
        with torch.no_grad():
            full = plan.run(x)
        torch.cuda.synchronize(DEV)
        assert torch.equal(full, pred), "the op-by-op walk must leave what a forward computes"
        kinds |= {o.kind for o in plan.ops}
        total_e += e
        total_l += launched
        print("plan %s B=%d %dx%d fuse=%r: %d ops, %d candidates, %d launched, %d run before" % (scale, B, H, W, fuse, len(plan.ops), e, launched, dup))
        del plan, m, pred, full
        torch.cuda.empty_cache()
    print("candidates enumerated %d, launched %d (distinct %d) in %.0f s" % (total_e, total_l, len(seen), time.time() - t0))
    for fam in sorted(stats):
        print("  %-44s %5d   max |got - ref| / bound %.3f" % (fam, stats[fam], worst[fam]))
    fams = set(stats)
    for tk in range(1, 9):
        assert any(" tile_k=%d " % tk in f for f in fams), tk
    for f in ("dw generic", "dw dot2", "dw pixel-pair", "dw pixel-pair staged", "dw matrix-core", "stem2 rows=4", "stem2 rows=8"):
        assert f in fams, f
    assert any(f.startswith("headtail") for f in fams)
    for k in (lib.OP_STEM2, lib.OP_BOTTLENECK, lib.OP_CONV1DW, lib.OP_SPPF_POOL, lib.OP_HEADTAIL, lib.OP_CONV1X1, lib.OP_CONV3X3S2, lib.OP_DWCONV):
        assert k in kinds and "plan config: " + _KIND[k] in fams, k


def test_the_checker_fails_a_stale_weight():
    """One tile_k = 8 candidate (DMA ring) and one pixel-pair candidate at a bench-shape op, with the last k-step (the last tap) of one output channel
    zeroed in their packed weights: the walk must reject both.  (Data only: the weights are edited before they are packed.)"""
    m = _model("n")
    plan = _plan(m, 32, 640, 640)
    x = O.synth_images(32, 640, seed=5).to(DEV).half()
    hit, failed, keep = {}, {}, []

    def dma(plan, i, c_):
        o, rec = plan.ops[i], plan._ops[i]
        if c_.tiles[2] != 8 or hit:
            return False
        w, b, srcC = rec["raw"]
        w = w.clone()
        kin = w.shape[1]
        last = (srcC[-1] if srcC else kin) - 1
        lo = kin - (last % 32 + 1)                                   # the input channels of the last k-step (each source is padded to whole k-steps)
        if o.kind == lib.OP_CONV3X3S2:
            w[0, lo:, 2, 2] = 0                                      # (tap-major: the last tap's last channels)
        else:
            w[0, lo:] = 0
        wp, bp = tuner.packed(plan, i, w, b, c_.tiles[1], 8)
        keep.extend([wp, bp])
        c_.op.w = wp.data_ptr()
        hit["dma"] = (plan.op_names[i], c_.tiles)
        return True

    def pairs(plan, i, c_):
        if not c_.pairs or hit:
            return False
        w = plan._ops[i]["raw"][0].clone()
        k = w.shape[-1]
        w[0, 0, k - 1, k - 1] = 0                                     # channel 0, the last tap
        wq = pack.pack_dw_pairs(w).to(DEV)
        keep.append(wq)
        c_.op.aux[1] = wq.data_ptr()
        hit["pairs"] = (plan.op_names[i], c_.tiles)
        return True

    for name, mut in (("dma", dma), ("pairs", pairs)):
        hit.clear()
        try:
            walk(plan, x, set(), {}, {}, mutate=mut)
        except AssertionError as e:
            failed[name] = (hit.get(name), str(e)[:200])
        assert name in hit and name in failed, (name, hit, failed)
    print(failed)


@pytest.mark.parametrize("scale,table", [("n", "round6_tune.json"), ("s", "round6_tune_s.json"), ("m", "round6_tune_m.json")])
def test_frozen_tables_pick_candidates_and_their_plans_predict_alike(scale, table):
    """The plan bench.py times: its committed table loaded, 32 x 640^2, autotune on.  Every committed pick of an op in it is one of that op's candidates;
    signatures the table lacks (timed at start-up) are listed; the predictions equal the oracle's on 2 images (_close16) and the
    untuned fp16 plan's on all 32 within twice that bar."""
    import json
    import os
    from test_gpu_model import _TOL16, _close16
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", table)
    saved = dict(tuner._TUNE_CACHE)
    try:
        tuner._TUNE_CACHE.clear()
        engine.load_tune_cache(path)
        frozen = dict(tuner._TUNE_CACHE)
        assert len(frozen) == len(json.load(open(path)))
        x = O.synth_images(32, 640, seed=1).to(DEV).half()
        m = M.Model(scale)
        m.load_state_dict(O.synth_state_dict(scale, 0))
        m = m.to(DEV).eval()
        m.autotune = True
        with torch.no_grad():
            got = m(x)[0].float().cpu().numpy()
        plan = m.plan_for(x)
        missing, checked = [], 0
        for i, o in enumerate(plan.ops):
            sig = tuner.signature(plan, i)
            if sig is None:
                continue
            if sig not in frozen:
                missing.append((plan.op_names[i], sig))
                continue
            tiles = [c_.tiles for c_ in (_dw_tiles_with_pairs(plan, i) if o.kind == lib.OP_DWCONV else tuner.candidates(plan, i))]
            picks = [frozen[sig]] + ([frozen[sig + ("nhwc",)]] if sig + ("nhwc",) in frozen else [])
            for p in picks:
                assert tuple(p) in tiles, (plan.op_names[i], sig, p)
                checked += 1
        print("%s: %d committed picks are candidates; signatures not in the table (timed at start-up): %s" % (table, checked, missing or "none"))
        assert checked >= len(plan.ops) // 3
    finally:
        tuner._TUNE_CACHE.clear()
        tuner._TUNE_CACHE.update(saved)
    # against the untuned fp16 plan on all 32 images within the sum of the two plans' fp16 bars: each fp16 plan rounds at its own points (fused
    # bottlenecks, MPRep in one launch, pixel pairs), so their gap is not one bar (m: one score among its 21.8 M score values lies 0.0093 from the untuned plan's, against 0.009)
    ref = M.Model(scale)
    ref.load_state_dict(O.synth_state_dict(scale, 0))
    ref = ref.to(DEV).eval()
    with torch.no_grad():
        base = ref(x)[0].float().cpu().numpy()
    assert np.isfinite(got).all()
    box_atol, score_atol = _TOL16[scale]
    np.testing.assert_allclose(got[..., :4], base[..., :4], rtol=5e-3, atol=2 * box_atol)
    np.testing.assert_allclose(got[..., 4:], base[..., 4:], rtol=0, atol=2 * score_atol)
    oracle = O.predict(O.reparam(O.synth_state_dict(scale, 0), scale), scale, x[:2].float().cpu()).numpy()
    _close16(got[:2], oracle, scale)


def test_time_candidates_skips_or_raises_a_rejected_launch():
    """tuner.time_candidates under the two policies of its call sites, at the smallest 1x1 conv that reaches both (1 x 4 x 4, 64 -> 32): the generic kernel, and
    CONV_STREAM_LDS with tile_c = 3, which the dispatcher turns down while it checks its arguments (MAF_E_UNSUPPORTED: nothing is launched).  The training
    tuners skip such a candidate, the inference tuner raises."""
    B, H, W, cin, cout = 1, 4, 4, 64, 32
    cands = [(1, 2, lib.CONV_GENERIC), (1, 3, lib.CONV_STREAM_LDS)]
    torch.manual_seed(0)
    x = torch.randn(B, cin, H, W, device=DEV).half().contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, cin, device=DEV) / cin ** 0.5
    out = torch.zeros(B, cout, H, W, device=DEV, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    wp, bp = train_ops._packed_1x1(w.contiguous(), cout, cin, 0, lib.F16, 2, DEV), train_ops._zero_bias(DEV, 64)
    st = train_ops._stream(DEV)

    def train_launch(c_):
        train_ops._launch_conv1x1(x, cin, wp, bp, B, H, W, cin, cout, c_[1], out, lib.F16, c_[0], c_[2])

    res = tuner.time_candidates(train_launch, cands, st, 3, "skip")
    torch.cuda.synchronize(DEV)
    assert len(res) == 1 and res[0][1] == cands[0] and res[0][0] > 0, res
    ref = torch.nn.functional.conv2d(x.float(), w.half().float().reshape(cout, cin, 1, 1))
    assert (out.float() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item() + 2e-3

    ops = []
    for pt, ct, tk in cands:
        op = lib.MafOp()
        op.kind, op.dtype, op.in_dtype, op.act = lib.OP_CONV1X1, lib.F16, lib.F16, lib.ACT_NONE
        op.B, op.H, op.W, op.Cin, op.Cout, op.nsrc = B, H, W, cin, cout, 1
        op.src[0].ptr, op.src[0].C, op.src[0].stride, op.src[0].mode = x.data_ptr(), cin, cin, lib.SRC_DIRECT
        op.out, op.out_stride, op.w, op.bias = out.data_ptr(), cout, wp.data_ptr(), bp.data_ptr()
        op.tile_p, op.tile_c, op.tile_k = pt, ct, tk
        ops.append(op)
    L = lib.load()
    assert L.maf_op_launch(C.byref(ops[1]), st) == -2                  # MAF_E_UNSUPPORTED
    with pytest.raises(lib.MafError):
        tuner.time_candidates(lambda op: lib.check(L.maf_op_launch(C.byref(op), st)), ops, st, 5, "raise")
    torch.cuda.synchronize(DEV)
