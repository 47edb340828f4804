"""Measured choices of a launch plan (engine.Plan): which fusion mode every DepthBottleneckUni takes (`choose_fusion`), which (pixels x channels) tile / kernel variant
every conv and depth-wise launch takes (`autotune`), and the cache that freezes them (`save_tune_cache` / `load_tune_cache`: profiles/round*_tune*.json).

Split out of engine.py in round 6 (engine.py = the plan: graph -> launch list -> C engine; this file = what is timed on the device; plan_report.py = what a plan
says about itself: kernel names, algorithmic bytes, flops).  The reference has no counterpart: it leaves kernel selection to cuDNN / MIOpen heuristics per call
(yolov6/layers/common.py:29-50 calls nn.Conv2d)."""
import ctypes as C
import os

import torch

from .config import cfg
from . import conv_variants, lib, pack
from .conv_variants import stream_lds_ok, time_candidates      # noqa: F401  (re-exported)

_TUNE_CACHE = {}          # layer signature -> (tile_p, tile_c, ...), filled by autotune


def choose_fusion(model, B, H, W, dtype, in_dtype, device, x, reps=3):
    """Measure, per DepthBottleneckUni, the three ways of running it on this device — three launches, the fully fused kernel
    (c <= 64), conv1+depth-wise fused followed by the plain 1x1 — and return {bottleneck name: mode}.  Decisions are cached by layer
    signature next to the tile choices."""
    import numpy as np
    # (the three ways are compared WITHOUT the block's closing conv inside the fused launch — fuse_tail — which the final plan adds wherever mode 1 wins)
    from .engine import Plan
    plan1 = Plan(model, B, H, W, dtype, in_dtype, device, fuse=True, fuse_tail=False)           # full fusion where it exists, partial elsewhere
    names, sigs = [], {}
    for i, o in enumerate(plan1.ops):
        nm = plan1.op_names[i]
        if o.kind == lib.OP_BOTTLENECK:
            names.append(nm); sigs[nm] = ("bn3", dtype, B, o.H, o.W, o.Cin, o.ksize)
        elif o.kind == lib.OP_CONV1DW:
            names.append(nm[:-len(".conv1dw")]); sigs[names[-1]] = ("bn3", dtype, B, o.H, o.W, o.Cin, o.ksize)
    if names and not all(sigs[n] in _TUNE_CACHE for n in names):
        pred = torch.empty(B, plan1.A, 5 + plan1.nc, dtype=torch.float32, device=device)

        def timed(plan):
            plan.autotune(x)
            plan.run_timed(x, pred)
            t = np.min([plan.run_timed(x, pred) for _ in range(reps)], 0)
            return dict(zip(plan.op_names, t))
        t0 = timed(Plan(model, B, H, W, dtype, in_dtype, device, fuse=False, fuse_tail=False))
        t1 = timed(plan1)
        t2 = timed(Plan(model, B, H, W, dtype, in_dtype, device, fuse=2, fuse_tail=False))
        for n in names:
            cost = {0: t0[n + ".conv1"] + t0[n + ".conv2"] + t0[n + ".one_conv"], 2: t2[n + ".conv1dw"] + t2[n + ".one_conv"]}
            if n in t1:
                cost[1] = t1[n]
            _TUNE_CACHE[sigs[n]] = (min(cost, key=cost.get),)
    del plan1
    return {n: _TUNE_CACHE[sigs[n]][0] for n in names}


def save_tune_cache(path):
    """Persist the tile choices found by Plan.autotune (JSON: repr(signature) -> tiles) so a later process — a profiler
    pass, a serving replica — builds byte-identical plans without re-timing."""
    import json
    with open(path, "w") as f:
        json.dump({repr(k): list(v) for k, v in _TUNE_CACHE.items()}, f, indent=0, sort_keys=True)


def load_tune_cache(path):
    import ast
    import json
    with open(path) as f:
        for k, v in json.load(f).items():
            _TUNE_CACHE[ast.literal_eval(k)] = tuple(v)
    return len(_TUNE_CACHE)
# lanes served together by one ds_read_b128 (four groups of 16): what the LDS pitch searches below count bank-slot collisions over
_LANE_GROUPS = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31),
              (32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59), (36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63))


_P2_STAGE = cfg.dw_stage      # A/B switch of the tuner's staged-store candidates for dwconv_p2 (tile_k + 128)


def p2_wave_bytes(th, tw, k):
    """LDS bytes of one wave of dwconv_p2 (two planes of 16-byte pair slots, whole DMA rounds): csrc/dwconv_p2.hip:p2_pitch / maf_launch_dwconv_p2."""
    p_ = k // 2
    pe = p_ + (p_ & 1)
    rwp, spr = tw // 2 + pe, tw // 4
    nstrips = th * spr
    best, bc = rwp, 1 << 30
    for pitch in range(rwp, rwp + 8):
        c = 0
        for g in _LANE_GROUPS:
            cnt = {}
            for lane in g:
                s_ = min(lane, nstrips - 1)
                slot = ((s_ // spr) * pitch + 2 * (s_ % spr)) & 15
                cnt[slot] = cnt.get(slot, 0) + 1
            c += max(cnt.values())
        if c < bc:
            best, bc = pitch, c
    return -(-(2 * (th + k - 1) * best) // 64) * 1024



_TUNED_KINDS = (lib.OP_STEM2, lib.OP_HEADTAIL, lib.OP_DWCONV, lib.OP_CONV1X1, lib.OP_CONV3X3S2)


class Candidate:
    """One launch the tuner times for an op.  `tiles`: what `_TUNE_CACHE` stores for it ((rows, 0, workgroups) of a stem pair, (0, 0, iterations) of a head tail,
    (tile_p, tile_c, tile_k) otherwise); `op`: a copy of the plan's MafOp with the candidate's tile fields, packed weights / bias and twin operands; `keep`: the
    tensors `op` points into; `pairs`: the op reads its source as pixel pairs (src[0].mode = SRC_PAIRS), so in a plan its producer stores them (out_pairs = 1)."""
    __slots__ = ("tiles", "op", "keep", "pairs")

    def __init__(self, tiles, op, keep=(), pairs=False):
        self.tiles, self.op, self.keep, self.pairs = tuple(tiles), op, list(keep), pairs

    def __repr__(self):
        return "Candidate(%r%s)" % (self.tiles, ", pairs" if self.pairs else "")


def _feeds_pairs(plan, i):
    # a 1x1 conv whose only reader is a depth-wise conv can hand it PIXEL PAIRS — but only from the LDS-resident-weight kernel (CONV_STREAM_LDS)
    o = plan.ops[i]
    if not (o.kind == lib.OP_CONV1X1 and i + 1 < len(plan.ops) and plan.ops[i + 1].kind == lib.OP_DWCONV):
        return False
    keep_tk, o.tile_k = o.tile_k, lib.CONV_STREAM_LDS
    try:
        return plan._pairs_producer(i + 1) is not None
    finally:
        o.tile_k = keep_tk


def signature(plan, i):
    """The `_TUNE_CACHE` key of op i of `plan`, or None for an op the tuner does not time."""
    o, r = plan.ops[i], plan._ops[i]
    if o.kind == lib.OP_STEM2:
        return (o.kind, plan.dtype, plan.in_dtype, plan.B, o.H, o.W, o.ksize, o.Cout, o.nc)
    if o.kind == lib.OP_HEADTAIL:
        return (o.kind, plan.dtype, plan.B, o.H, o.W, o.Cin, "percu")
    if o.kind == lib.OP_DWCONV:
        return (o.kind, plan.dtype, plan.B, o.H, o.W, o.Cin, o.ksize, o.act) + ((o.Cout,) if o.Cout != o.Cin else ())
    if o.kind not in (lib.OP_CONV1X1, lib.OP_CONV3X3S2):
        return None
    M = plan.B * o.H * o.W
    return (o.kind, plan.dtype, M, o.Cin, o.Cout, o.nsrc, tuple(o.src[k].mode for k in range(o.nsrc)), int(o.out_f32)) + (("twin",) if r.get("twin") else ()) \
        + (("pool1",) if r.get("pool1") else ()) + (("pairs",) if _feeds_pairs(plan, i) else ())


_FUSED_3X3 = (lib.CONV3_LDS, lib.CONV3_WREG)      # their weight record holds the bias and does not depend on tile_c


def packed(plan, i, wt, bt, ct, tk):
    """(weights, bias) of conv op i packed for tile_c = ct, tile_k = tk (device tensors; one record with the bias inside for CONV3_LDS / CONV3_WREG)."""
    o, r = plan.ops[i], plan._ops[i]
    pool1, srcC = r.get("pool1"), r["raw"][2]
    wreg = tk == lib.CONV3_WREG
    wp_ = ((pack.pack_mprep_wreg if wreg else pack.pack_mprep_lds)(wt, bt, *pool1) if pool1 else pack.pack_conv3x3_lds(wt, bt) if tk == lib.CONV3_LDS else pack.pack_conv3x3_wreg(wt, bt) if wreg
           else pack.pack_conv1x1(wt, srcC, ct, plan.dtype) if o.kind == lib.OP_CONV1X1 else pack.pack_conv3x3(wt, ct, plan.dtype)).to(plan.device)
    return wp_, pack.pack_bias(bt, ct if tk not in _FUSED_3X3 else 4).to(plan.device)


def conv_tiles(plan, i):
    """(tile_p, tile_c, tile_k) of every variant the tuner times for conv op i (OP_CONV1X1 / OP_CONV3X3S2), in timing order: conv_variants.conv_tiles of the op."""
    o, r = plan.ops[i], plan._ops[i]
    return conv_variants.conv_tiles(o.kind, plan.dtype, plan.B * o.H * o.W, [(o.src[k].C, o.src[k].mode) for k in range(o.nsrc)], o.Cout, o.out_stride, bool(o.out_f32),
                                    bool(r.get("twin")), r.get("pool1_tk", lib.CONV3_LDS) if r.get("pool1") else None)


def dw_tiles(plan, i):
    """(tile_p, tile_c, tile_k) of every variant the tuner times for depth-wise op i, in timing order: the v_fma_mix kernel's (rows, columns, channel block), then
    dot2 (DW_DOT2), pixel pairs (DW_PAIRS; only where the 1x1 conv in front, as the plan stands, can store pairs) and the matrix-core form (DW_MFMA); the tile_k
    of dot2 / pairs: lib.dw_tile_k."""
    o = plan.ops[i]
    n = 8 if plan.dtype == lib.F16 else 4
    out = []
    # tile heights / widths: powers of two plus the map's own size and its half (40 x 40 and 20 x 20 maps: tiles that
    # divide the map exactly have no half-empty edge tiles and the smallest halo share)
    ths = sorted({4, 8, 16, 32} | {v for v in (o.H, o.H // 2) if 8 <= v <= 40})
    tws = sorted({8, 16, 32} | {v for v in (o.W, o.W // 2) if 8 <= v <= 40 and v % 4 == 0})
    for th in ths:
        for tw in tws:
            for cbm in (8, 4, 2):
                t_h, t_w, cb = min(th, o.H), min(tw, -(-o.W // 4) * 4), min(cbm * n, -(-o.Cin // n) * n)
                lds = ((t_h + o.ksize - 1) * (t_w + o.ksize - 1) * (cb // n + 2) + o.ksize * o.ksize * (cb // n)) * 16
                if lds > 96 * 1024 or (t_h, t_w, cb) in out:
                    continue
                out.append((t_h, t_w, cb))
    if plan.dtype == lib.F16:                            # two taps per instruction (csrc/dwconv_dot2.hip): tile_c = columns, tile_k = rows, channels
        w8 = -(-o.W // 8) * 8
        for th in sorted({4, 8, 10, 16, 20} | ({o.H} if o.H <= 40 else set())):
            if th > o.H:
                continue
            for tw in sorted({16, 24, 32, 40} | ({w8} if w8 <= 40 else set())):
                if tw > w8:
                    continue
                for cb in (16, 32, 64):
                    cb = min(cb, o.Cin)
                    nq, np_ = cb // 4, (o.ksize + 1) // 2
                    lds = ((th + o.ksize - 1) * ((tw + o.ksize - 1) // 2) * (nq + 3) + o.ksize * 2 * np_ * nq) * 16      # (pair stride <= nq + 3: csrc/dwconv_dot2.hip)
                    if lds > 96 * 1024 or (lib.DW_DOT2, tw, lib.dw_tile_k(th, cb)) in out:
                        continue
                    out.append((lib.DW_DOT2, tw, lib.dw_tile_k(th, cb)))
    if plan._pairs_producer(i) is not None:              # pixel-pair input, v_dot2c with scalar weight pairs (csrc/dwconv_p2.hip): tile_c = columns, tile_k = rows, waves per workgroup
        w4 = -(-o.W // 4) * 4
        for th in sorted({4, 5, 8, 10, 16, 20} | ({o.H} if o.H <= 40 else set())):
            if th > o.H:
                continue
            for tw in sorted({16, 20, 32, 40, 80} | ({w4} if w4 <= 80 else set())):
                if tw > w4:
                    continue
                plane = p2_wave_bytes(th, tw, o.ksize)
                if plane > 20 * 1024:                    # fewer than 8 waves per CU: never the fastest
                    continue
                for nw, stg in ((2, False), (4, False), (8, False), (2, True), (4, True), (8, True)):
                    # staged stores (the waves of a workgroup = adjacent channel groups of one tile, results through the dead planes,
                    # nw x 16-byte runs per pixel): where the kernel takes that form (csrc/dwconv_p2.hip:maf_launch_dwconv_p2)
                    if stg and not ((o.Cin // 8) % nw == 0 and th * (tw // 4) <= 64 and plane >= 4160 and o.Cout <= 2 * o.Cin and _P2_STAGE):
                        continue
                    out.append((lib.DW_PAIRS, tw, lib.dw_tile_k(th, nw, stg)))
    if plan.dtype == lib.F16 and o.aux[0]:               # matrix-core variant (csrc/dwconv_mfma.hip)
        out.append((lib.DW_MFMA, 0, 0))
    return out


def candidates(plan, i):
    """Every launch the tuner times for op i of `plan`, in timing order (a list of `Candidate`; empty for an op it does not time).  Stem pairs: tile height (8 / 4
    rows; 4 only for the 48 -> 96 stem, whose kernel takes no other) x persistent workgroups; head tails: persistent iterations per CU; depth-wise: `dw_tiles`;
    1x1 and 3x3 stride-2 convs: `conv_tiles`, each with its own weight packing.  The list of a depth-wise op depends on the tile_k its producer holds (pixel pairs
    only behind CONV_STREAM_LDS), so it is what the tuner offers at the point it reaches op i.  The stem's image (src[0].ptr) and the head tail's output are the plan
    op's: the caller points them at real buffers."""
    o, r = plan.ops[i], plan._ops[i]
    if o.kind == lib.OP_STEM2:
        out = []
        for rows in ((4,) if o.Cout == 96 else (8, 4)):
            for wgs in (256, 512, 768, 1024):
                op = lib.MafOp.from_buffer_copy(o)
                op.tile_p, op.tile_k = rows, wgs
                out.append(Candidate((rows, 0, wgs), op))
        return out
    if o.kind == lib.OP_HEADTAIL:
        out = []
        for iters in (1, 2, 3, 4, 6):
            op = lib.MafOp.from_buffer_copy(o)
            op.tile_k = iters
            out.append(Candidate((0, 0, iters), op))
        return out
    if o.kind == lib.OP_DWCONV:
        out = []
        for tp, tc, tk in dw_tiles(plan, i):
            op = lib.MafOp.from_buffer_copy(o)
            op.tile_p, op.tile_c, op.tile_k = tp, tc, tk
            op.src[0].mode = lib.SRC_PAIRS if tp == lib.DW_PAIRS else lib.SRC_DIRECT
            out.append(Candidate((tp, tc, tk), op, pairs=tp == lib.DW_PAIRS))
        return out
    if o.kind not in (lib.OP_CONV1X1, lib.OP_CONV3X3S2):
        return []
    w, b = r["raw"][:2]
    twin = r.get("twin")
    packs, out = {}, []
    for pt, ct, tk in conv_tiles(plan, i):
        form = (0, tk) if tk in _FUSED_3X3 else (ct, 0)
        if form not in packs:
            packs[form] = packed(plan, i, w, b, ct, tk) + (packed(plan, i, *twin["raw"], ct, tk) if twin else ())
        keep = packs[form]
        op = lib.MafOp.from_buffer_copy(o)
        op.tile_p, op.tile_c, op.tile_k, op.w, op.bias = pt, ct, tk, keep[0].data_ptr(), keep[1].data_ptr()
        op.out_pairs = 0
        if twin:
            op.aux[1], op.aux[2] = keep[2].data_ptr(), keep[3].data_ptr()
        out.append(Candidate((pt, ct, tk), op, keep))
    return out


def autotune(plan, x, reps=5, verbose=False):
    """Time every candidate (`candidates`) of every stem pair, head tail, depth-wise and MFMA conv launch on this device and keep the fastest.
    The candidates differ only in how the work is cut into wave tiles / workgroups (and in the matching weight packing); results are cached per
    layer signature in `_TUNE_CACHE` so other plans of the same model reuse them."""
    assert x.is_cuda
    L = lib.load()
    stream = torch.cuda.current_stream(plan.device)
    pred = torch.empty(plan.B, plan.A, 5 + plan.nc, dtype=torch.float32, device=plan.device)
    plan.run_into(x, pred)                                   # every buffer holds realistic data
    torch.cuda.synchronize(plan.device)
    plan._tuned = getattr(plan, "_tuned", [])
    changed = 0

    def timed(cands):
        res = time_candidates(lambda c_: lib.check(L.maf_op_launch(C.byref(c_.op), stream.cuda_stream)), cands, stream.cuda_stream, reps, "raise")
        return [(t,) + c_.tiles for t, c_ in res]

    for i, (o, r) in enumerate(zip(plan.ops, plan._ops)):
        sig = signature(plan, i)
        if sig is None:
            continue
        best = _TUNE_CACHE.get(sig)
        if o.kind == lib.OP_STEM2:                           # stem pair: tile height (8 / 4 rows) and number of persistent workgroups
            if best is None:
                o.src[0].ptr = x.data_ptr()
                results = sorted((t, rows, wgs) for t, rows, _, wgs in timed(candidates(plan, i)))
                best = (results[0][1], 0, results[0][2])
                _TUNE_CACHE[sig] = best
                if verbose:
                    print("tune %-32s %dx%d: %s" % (plan.op_names[i], o.H, o.W, " ".join("(%d,%d)%.1fus" % (r_, w_, t * 1e3) for t, r_, w_ in results)))
            if (best[0], best[2]) != (o.tile_p, o.tile_k):
                o.tile_p, o.tile_k = best[0], best[2]
                changed += 1
            continue
        if o.kind == lib.OP_HEADTAIL:                        # head tail: persistent workgroups per CU (tile_k; the weights are staged once per workgroup)
            if best is None:
                o.out = pred.data_ptr()
                results = sorted((t, it) for t, _, _, it in timed(candidates(plan, i)))
                best = (0, 0, results[0][1])
                _TUNE_CACHE[sig] = best
                if verbose:
                    print("tune %-32s %dx%d C=%d: %s" % (plan.op_names[i], o.H, o.W, o.Cin, " ".join("(%d)%.1fus" % (it, t * 1e3) for t, it in results)))
            if best[2] != o.tile_k:
                o.tile_k = best[2]
                changed += 1
            continue
        if o.kind == lib.OP_DWCONV:                          # depth-wise: workgroup tile (rows, cols, channel block)
            if best is None:
                results = sorted(timed(candidates(plan, i)))     # (pixel-pair candidates read the NHWC content of the buffer as pairs: same work)
                best = results[0][1:]
                _TUNE_CACHE[sig] = best
                _TUNE_CACHE[sig + ("nhwc",)] = [r_ for r_ in results if r_[1] != lib.DW_PAIRS][0][1:]      # for a plan whose producer cannot store pixel pairs
                if verbose:
                    print("tune %-32s %dx%d C=%d k=%d: %s" % (plan.op_names[i], o.H, o.W, o.Cin, o.ksize, " ".join("(%d,%d,%d)%.1fus" % (a, b2, c2, t * 1e3) for t, a, b2, c2 in results[:6])))
                    p2 = [r_ for r_ in results if r_[1] == lib.DW_PAIRS]
                    if any(r_[3] & lib.DW_P2_STAGED for r_ in p2):   # pixel-pair kernel: best tile with plain / staged stores
                        bu, bs = [r_ for r_ in p2 if not r_[3] & lib.DW_P2_STAGED][0], [r_ for r_ in p2 if r_[3] & lib.DW_P2_STAGED][0]
                        print("     dwconv_p2 stores  plain (%d,%d) %.1fus   staged (%d,%d) %.1fus" % (bu[2], bu[3], bu[0] * 1e3, bs[2], bs[3] - lib.DW_P2_STAGED, bs[0] * 1e3))
            prod = plan._pairs_producer(i)
            if best[0] == lib.DW_PAIRS and prod is None:
                best = _TUNE_CACHE.get(sig + ("nhwc",), (0, 0, 0))
            pairs = 1 if best[0] == lib.DW_PAIRS else 0
            if tuple(best) != (o.tile_p, o.tile_c, o.tile_k) or (prod is not None and prod.out_pairs != pairs):
                o.tile_p, o.tile_c, o.tile_k = best
                o.src[0].mode = lib.SRC_PAIRS if pairs else lib.SRC_DIRECT
                if prod is not None:
                    prod.out_pairs = pairs                           # the 1x1 conv in front stores what this kernel reads
                changed += 1
            continue
        twin, pool1 = r.get("twin"), r.get("pool1")
        if best is None:
            results = sorted(timed(candidates(plan, i)))
            best = (results[0][1], results[0][2], results[0][3])
            # where pairs are possible (signature: "pairs"), CONV_STREAM_LDS is kept unless another variant is clearly (1.3x) faster.  Timed alone, the register-weight form
            # sometimes wins such a layer by a few hundred nanoseconds (run-to-run noise) and the depth-wise conv behind it then loses its pair input
            # (n, 20 x 20 x 288, k = 9: 20.9 -> 27.9 us)
            if sig[-1] == "pairs":
                five = [r_ for r_ in results if r_[3] == lib.CONV_STREAM_LDS]
                if five and five[0][0] <= 1.3 * results[0][0]:
                    best = (five[0][1], five[0][2], five[0][3])
            _TUNE_CACHE[sig] = best
            if verbose:
                M = plan.B * o.H * o.W
                print("tune %-32s M=%-7d %4d->%-4d: %s" % (plan.op_names[i], M, o.Cin, o.Cout, " ".join("(%d,%d%s)%.1fus" % (p, c, "," + lib.CONV_VARIANT_NAMES[k] if k > lib.CONV_GENERIC else "", t * 1e3) for t, p, c, k in results)))
        pt, ct, tk = best
        if pool1:
            if (pt, ct) != (o.tile_p, o.tile_c):
                o.tile_p, o.tile_c = pt, ct                       # same record, another workgroup count
                changed += 1
            continue
        if (pt, ct, tk) != (o.tile_p, o.tile_c, max(1, o.tile_k)):
            wp, bp = packed(plan, i, *r["raw"][:2], ct, tk)
            plan._tuned += [wp, bp]
            o.tile_p, o.tile_c, o.tile_k, o.w, o.bias = pt, ct, tk, wp.data_ptr(), bp.data_ptr()
            if twin:
                wp2, bp2 = packed(plan, i, *twin["raw"], ct, tk)
                plan._tuned += [wp2, bp2]
                o.aux[1], o.aux[2] = wp2.data_ptr(), bp2.data_ptr()
            changed += 1
    if changed:
        L.maf_engine_destroy(plan._engine)
        h = C.c_void_p()
        lib.check(L.maf_engine_create(plan.ops, len(plan.ops), C.byref(h)))
        plan._engine = h
    torch.cuda.synchronize(plan.device)
    return changed
