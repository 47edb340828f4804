"""Which launches of the matrix-core convs are worth timing for a layer shape, and the loop that times them: the one rule set behind the inference tuner
(tuner.conv_tiles), the training 1x1 tuner (train_ops.conv_candidates) and the training 3x3 stride-2 tuners (train_conv).  A leaf module: lib and pack only."""
from . import lib, pack


def stream_lds_ok(ksteps, ct):
    """Instantiations of the persistent 1x1 conv with LDS-resident weights (CONV_STREAM_LDS: csrc/conv_stream_lds.hip, conv_stream_lds_wide.hip)."""
    if 2 <= ksteps <= 12:
        return ksteps * ct <= 96
    if ct == 4 and ksteps in (26, 28, 30, 32, 34, 36, 40):          # conv_stream_lds_xwide.hip (round 6: the 832 ... 1280-channel reductions of s / m)
        return True
    return ct in (4, 6, 8) and (13 <= ksteps <= 20 or ksteps == 24) and ksteps * ct <= 160


def conv_tiles(kind, dtype, M, srcs, cout, out_stride, out_f32=False, twin=False, pool1_tk=None, fused_3x3=True):
    """(tile_p, tile_c, tile_k) of every variant worth timing for a conv (OP_CONV1X1 / OP_CONV3X3S2) over M output pixels, in timing order.  srcs: (channels, SRC_*
    mode) of every source; twin: a twin launch; pool1_tk: the op is a whole MPRep on that variant (only its workgroup count is open); fused_3x3: offer the
    CONV3_LDS / CONV3_WREG kernels (their records hold the bias: the training convs have none)."""
    f16, one, conv3 = dtype == lib.F16, len(srcs) == 1, kind == lib.OP_CONV3X3S2
    cin, modes = sum(c for c, _ in srcs), [m for _, m in srcs]
    f16out = f16 and not out_f32
    ksteps = sum(-(-c // (32 if f16 else 16)) for c, _ in srcs) * (9 if conv3 else 1)
    direct = not conv3 and one and modes[0] == lib.SRC_DIRECT
    cands = []
    for ct in (2, 4, 6, 8):
        nt = -(-cout // (16 * ct))
        if nt * 16 * ct > 2 * max(cout, 32) or (ct == 8 and out_stride % 8 and f16out):
            continue
        for pt in (1, 2, 4):
            if pt == 4 and ct > 4:
                continue
            if -(-M // (64 * pt)) * nt < 256 and pt > 1:
                continue                          # would not fill the chip
            cands.append((pt, ct, lib.CONV_GENERIC))
        if ksteps >= 8 and M <= 65536:
            cands.append((1, ct, lib.CONV_SPLITK))           # split-K across the 4 waves: long reductions on small maps
        if direct and f16out and ksteps <= 4 and ksteps * ct <= 16:
            for pt in (1, 2):                                # persistent waves, next tile's activations in flight during the epilogue
                cands.append((pt, ct, lib.CONV_STREAM))
        if not conv3 and f16out and stream_lds_ok(ksteps, ct) and (one or lib.SRC_POOL2 not in modes) and (direct or ct >= 4 or one):
            cands.append((1, ct, lib.CONV_STREAM_LDS))       # persistent waves, the channel tile's weights resident in LDS
            if ct >= 4 and 64 <= ksteps * ct <= 160 and (8 <= ksteps <= 20 or ksteps == 24):
                cands.append((2, ct, lib.CONV_STREAM_LDS))   # ... eight waves behind one copy of the weights where the LDS leaves room for one or two workgroups per CU (conv_stream_lds_w8.hip)
        if conv3 and fused_3x3 and f16 and ct == 4:
            if (cin, cout) in ((48, 48), (48, 64), (64, 64)) and (M >= 65536 or pool1_tk is not None):
                for wg in (4, 8, 12, 16):                     # weights + input patch in LDS, 256 .. 1024 persistent workgroups (tile_c = workgroups / 64)
                    cands.append((4, wg, lib.CONV3_LDS))
            if pack.conv3x3_wreg_shape(cin, cout):
                for wg in (2, 4, 8):                          # weights in registers, patches by DMA: 64 / 128 / 256 workgroups per conv (tile_c = that / 32)
                    if wg * 32 * (2 if twin else 1) <= 256:
                        cands += [(3, wg, lib.CONV3_WREG), (2, wg, lib.CONV3_WREG)]   # tile_p = patch buffers (3: two patches in flight ahead of the multiply)
        pooled = one and modes[0] == lib.SRC_POOL2
        if ksteps >= 4 and ct >= 4 and f16out and not pooled:
            for pt in ((1, 2, 4) if ct == 4 else (1, 2)):     # the workgroup shares each k-step's weight fragments through LDS
                if pt == 1 or -(-M // (64 * pt)) * nt >= 256:
                    cands.append((pt, ct, lib.CONV_LDS))
                    if pt <= 2 and ksteps >= 8:                # ... that arrive by DMA, two k-steps per barrier, three stages ahead (K-heavy layers)
                        cands.append((pt, ct, lib.CONV_DMA))
    if twin:                                                  # the variants that take a twin launch
        cands = [c_ for c_ in cands if c_[2] in (lib.CONV_GENERIC, lib.CONV_LDS, lib.CONV_SPLITK, lib.CONV3_WREG, lib.CONV_DMA)]
    if pool1_tk is not None:                                  # only the workgroup count (and the patch buffers of CONV3_WREG) are open
        cands = [c_ for c_ in cands if c_[2] == pool1_tk]
    return cands


def with_static(cands, static):
    """`cands` with the caller's static-rule tile timed last if none of them is it (the training tuners)."""
    return cands if static in cands else cands + [static]


def conv3_dgrad_tiles(cin, M, static):
    """(tile_p, tile_c, 0) of every launch timed for the data gradient of a 3x3 stride-2 conv with `cin` input channels over M input pixels
    (csrc/conv_mfma_dgrad.hip: tiles of 64 * tile_p pixels, tile_c in {2, 4, 8}; the library has tile_p 1 and 2 and refuses 4), then `static`."""
    cands = []
    for ct in (2, 4, 8):
        nt = -(-cin // (16 * ct))
        if nt * 16 * ct > 2 * max(cin, 32):
            continue
        for pt in (1, 2, 4):
            if (pt == 4 and ct > 4) or (pt > 1 and -(-M // (128 * pt)) * nt < 256):
                continue
            cands.append((pt, ct, 0))
    return with_static(cands, static)


def time_candidates(launch, cands, stream, reps, on_error):
    """[(fastest of `reps` timed launches in ms, candidate), ...] in the order of `cands`: launch(c) once to warm up, then `reps` times between HIP events on
    `stream` (a raw handle).  A candidate whose warm-up raises MafError is left out (on_error = "skip") or ends the timing (on_error = "raise")."""
    assert on_error in ("skip", "raise")
    timer, res = lib.Timer(), []
    for c_ in cands:
        try:
            launch(c_)
        except lib.MafError:
            if on_error == "skip":
                continue
            raise
        ts = []
        for _ in range(reps):
            timer.start(stream)
            launch(c_)
            timer.stop(stream)
            ts.append(timer.elapsed_ms())
        res.append((min(ts), c_))
    return res
