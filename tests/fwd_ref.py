"""EVERY case tests/test_gpu_fwd_edges.py runs on the forward (inference) kernels, as data, and their fp64 references.  Device-agnostic torch; checked on the CPU by
tests/test_fwd_ref_host.py on the very tensors the GPU test uses.

The references are tests/op_ref.py's (`op_ref.reference`, the restatement the tuner-candidate suite uses), called with a plain record of the case's operands in
place of a plan's: the 1x1 conv over concatenated SRC_DIRECT / SRC_UP2 / SRC_POOL2 / SRC_SUB2 sources, the 3x3 stride-2 conv (twin, pooled 1x1 branch), the
depth-wise conv (one or two filters per input channel), the stem conv and SPPF's three max-pools.  They share no index arithmetic with the kernels.

Two families, as in tests/wgrad_ref.py and tests/dgrad_ref.py.  Family E (exact): `int_case` activations, integer weights, an integer (or zero) bias, ACT_NONE or
ACT_RELU — every product and partial sum is an integer below 2^22, the fp32 accumulation is exact in any order and an fp16 store of an integer of magnitude <= 2048
is exact: the kernel must return THE integer, torch.equal(got, ref.to(dtype)).  Family B (bound): `wide_case` inputs, SiLU / sigmoid epilogues and u8 images, checked
against op_ref's per-element bound with its constants as they stand.

`CASES`: a list of dicts (name, kind, family, dtype, shape, seed, `why`: the branch of the dispatch the case exists for, `muts`: the mutations of `MUTATIONS` that
exist in it).  `inputs(case)` draws the tensors with a CPU generator; `reference(case, inp, mut)` is {output name: (ref, bound, S)}, optionally of a mutated input —
what test_fwd_ref_host.py uses to show that each case can tell a wrong kernel from a right one."""
import functools
from types import SimpleNamespace as NS

import torch

from maf_yolo_amd import lib

import op_ref
from dgrad_ref import _DW_C, _DW_MAPS, _M_BHW
from wgrad_ref import int_case, wide_case

D, UP2, POOL2, SUB2 = lib.SRC_DIRECT, lib.SRC_UP2, lib.SRC_POOL2, lib.SRC_SUB2
NONE, RELU, SILU, SIGMOID = lib.ACT_NONE, lib.ACT_RELU, lib.ACT_SILU, lib.ACT_SIGMOID
MUTATIONS = ("tap", "kstep", "row", "col", "batch", "up2", "pool2", "chunk", "div255")
M_BHW = dict(_M_BHW)
M_BHW[129] = (3, 1, 43)
del M_BHW[4551]
# The persistent 1x1 kernels launch ONE round of waves that stride over the 16 tile_p-pixel tiles.  conv_stream.hip: at most 1536 workgroups of 4 waves, rounded up
# to a multiple of the nN channel tiles (200 channels at tile_c 2: nN 7, 1540 workgroups, 880 waves per channel tile) — a wave gets a second tile past 880 tiles,
# 28160 pixels at tile_p = 2.  conv_stream_lds.inc.h: min(ceil(tiles / waves), occupancy (<= 4) * 256 / nN) workgroups per channel tile, at most 1024 * 8 waves
# (nN 1) — 28170 pixels are 1761 tiles of 16, more than the 4 x 146 waves nN = 7 leaves a channel tile.  28170 = 2 x 3 x 4695: the last tile of either holds 10 pixels.
PERSISTENT_BHW = (2, 3, 4695)
CASES = []


def src_grid(mode, H, W):
    """The grid of a source read through `mode` by an op whose own grid is H x W."""
    return (H // 2, W // 2) if mode == UP2 else (2 * H, 2 * W) if mode in (POOL2, SUB2) else (H, W)


def _muts(kind, kw):
    m = ["row", "col"]
    if kw["B"] >= 2:
        m.append("batch")
    if kind in ("conv3", "dw", "stem"):
        m.append("tap")
    if kind in ("conv1", "conv3"):
        m += ["kstep"] + (["chunk"] if kw["srcs"][0][0] >= 16 else [])
        modes = [s[1] for s in kw["srcs"]]
        if UP2 in modes and kw["W"] >= 4:                      # (a 1 x 1 source has one pixel at either parity)
            m.append("up2")
        if POOL2 in modes:
            m.append("pool2")
    if kind == "dw":
        m += ["kstep"] + (["chunk"] if kw["C"] >= 16 else [])
    if kind == "sppf":
        m += ["kstep"] + (["chunk"] if kw["C"] >= 16 else [])
    if kind == "fused":
        # one tap of the depth-wise filter under the closing conv: behind two more 1x1 convs and three fp16 rounding points it moves the result by less than the
        # three-stage bound (7 units of 2^-11 S) once the block is 48 channels wide — what op_ref's docstring says of long reductions; the 24- and 32-channel tails show it
        # (likewise 8 misread channels of 64 under the closing conv)
        m += ["kstep"] + (["chunk"] if kw["c"] >= 16 and (kw["sub"] != "tail" or kw["c"] <= 48) else []) + (["tap"] if kw["sub"] != "tail" or kw["c"] <= 32 else [])
    if kind == "head":
        m += ["kstep", "chunk"]
    if kind == "stem2":
        m.append("tap")
        if kw["third"] and kw["in_dtype"] == "u8":
            # three stages on an all-positive image: op_ref's chain on absolute values (4.75 units of 2^-11 S, S without any cancellation) is as large as the
            # outputs themselves, and of the mutations only the missing / 255 is past it (measured on the CPU: tap, row, column and batch swap move the reference by
            # 0.5 .. 1.8 bounds).  These three cases check the u8 load, the / 255 and the slices; the f16 / f32 cases of the same kernels see every mutation.
            m = []
    if kind in ("stem", "stem2") and kw["in_dtype"] == "u8":
        m.append("div255")
    return tuple(x for x in MUTATIONS if x in m)


def _case(kind, tag, why, family="E", dtype="f16", act=None, **kw):
    act = (NONE if len(CASES) % 2 else RELU) if act is None else act
    if (kind == "dw" or kw.get("cout") == 2) and act == RELU:     # (two channels under a ReLU: a dropped pixel may hide behind two zeros)
        act = NONE                                             # (and the depth-wise kernels take ACT_NONE and ACT_SILU only)
    assert (family == "E") == (act in (NONE, RELU)) or kind in ("sppf", "stem", "stem2")
    name = "%s-%s" % (kind, tag)
    CASES.append(dict(kind=kind, name=name, why=why, family=family, dtype=dtype, act=act, seed=4000 + len(CASES), muts=_muts(kind, kw), **kw))


def _bhw(M):
    return dict(zip("BHW", M_BHW[M]))


_M_WHY = {15: "M 15: one short of a 16-pixel tile", 16: "M 16: one 16-pixel tile", 17: "M 17: one pixel past a 16-pixel tile", 63: "M 63: one short of a 64-pixel tile",
          65: "M 65: one pixel past a 64-pixel tile", 129: "M 129: one pixel past a tile_p = 2 tile"}
_MS = (15, 16, 17, 63, 65, 129)

# ------------------------------------------------------------------------------------------------------------------------------------------- OP_CONV1X1
# every Cin against every Cout, the pixel counts rotating through them (each M meets each Cin or Cout class at least twice)
_CIN = [(8, "Cin 8: a quarter k-step"), (40, "Cin 40: a k-step and a quarter"), (72, "Cin 72: a partial third k-step"), (200, "Cin 200: a partial seventh k-step"),
        (64, "Cin 64: two whole k-steps")]
_COUT = [(2, "Cout 2: one partial channel tile"), (24, "Cout 24: a partial tile for every tile_c"), (68, "Cout 68: 4 channels into the last tile"), (200, "Cout 200: 8 into the last 32 / 64 / 96 / 128")]
for _i, (_ci, _cw) in enumerate(_CIN):
    for _j, (_co, _ow) in enumerate(_COUT):
        _M = _MS[(_i * 4 + _j) % 6]
        _case("conv1", "%dto%d-M%d" % (_ci, _co, _M), "%s; %s; %s" % (_cw, _ow, _M_WHY[_M]), srcs=[(_ci, D)], cout=_co, **_bhw(_M))
for _ci, _co, _M in [(8, 2, 17), (40, 24, 65), (72, 68, 15), (200, 200, 63), (64, 24, 129), (24, 68, 16)]:
    _case("conv1", "f32-%dto%d-M%d" % (_ci, _co, _M), "the fp32 instantiations (16-channel k-steps, 4-channel chunks); " + _M_WHY[_M], dtype="f32", srcs=[(_ci, D)], cout=_co, **_bhw(_M))
_case("conv1", "persistent-40to200", "CONV_STREAM (tile_p 1 and 2) and CONV_STREAM_LDS: 28170 pixels give some wave a second tile, and the last tile of all holds 10 pixels",
      srcs=[(40, D)], cout=200, only=(lib.CONV_STREAM, lib.CONV_STREAM_LDS), B=PERSISTENT_BHW[0], H=PERSISTENT_BHW[1], W=PERSISTENT_BHW[2])
# VAR_MULTI
_case("conv1", "multi2-2x2", "VAR_MULTI, two sources, the second through UP2 of a 1 x 1 map", srcs=[(40, D), (24, UP2)], cout=24, B=2, H=2, W=2)
_case("conv1", "multi2-6x10", "VAR_MULTI, two sources, UP2 first", srcs=[(72, UP2), (8, D)], cout=68, B=1, H=6, W=10)
_case("conv1", "multi3-2x2", "VAR_MULTI, three sources, UP2 in the middle with C = 40 (no multiple of 32)", srcs=[(72, D), (40, UP2), (8, D)], cout=68, B=2, H=2, W=2)
_case("conv1", "multi3-6x10", "VAR_MULTI, three sources, UP2 in the middle with C = 40; 12 k-steps: the LDS, DMA and split-K variants take it", srcs=[(200, D), (40, UP2), (72, D)], cout=200, B=2, H=6, W=10)
_case("conv1", "f32-multi3-6x10", "VAR_MULTI in fp32", dtype="f32", srcs=[(24, D), (12, UP2), (8, D)], cout=24, B=1, H=6, W=10)
# VAR_POOL2: pooled and sub-sampled single sources
for _mode, _mn in ((POOL2, "pool2"), (SUB2, "sub2")):
    for (_H, _W), _co in (((1, 1), 24), ((3, 5), 68)):
        _case("conv1", "%s-%dx%d" % (_mn, _H, _W), "VAR_POOL2 with SRC_%s: a %d x %d map of a %d x %d source" % (_mn.upper(), _H, _W, 2 * _H, 2 * _W), srcs=[(72, _mode)], cout=_co, B=2, H=_H, W=_W)
    _case("conv1", "%s-16wide" % _mn, "SRC_%s with a 16-wide source slice of a wider buffer (half a k-step), offered to CONV_STREAM_LDS too" % _mn.upper(), srcs=[(16, _mode)], cout=24, B=2, H=3, W=5,
          extra=[(1, 2, lib.CONV_STREAM_LDS), (1, 4, lib.CONV_STREAM_LDS)])
_case("conv1", "f32-pool2-3x5", "VAR_POOL2 in fp32", dtype="f32", srcs=[(24, POOL2)], cout=24, B=2, H=3, W=5)
# out_f32, out_pairs
_case("conv1", "outf32-72to68", "out_f32 on a partial channel tile and a partial pixel tile", srcs=[(72, D)], cout=68, out_f32=True, **_bhw(17))
_case("conv1", "outf32-264to2", "out_f32 with nine k-steps: the split-K form", srcs=[(264, D)], cout=2, out_f32=True, **_bhw(65))
_case("conv1", "pairs-W2", "out_pairs at W = 2: every pair is a whole row", srcs=[(72, D)], cout=24, out_pairs=True, only=(lib.CONV_STREAM_LDS,), B=2, H=3, W=2)
_case("conv1", "pairs-M30", "out_pairs at M = 30: even, no multiple of 16 — the last tile ends on a pair", srcs=[(72, D)], cout=68, out_pairs=True, only=(lib.CONV_STREAM_LDS,), B=1, H=5, W=6)
_case("conv1", "pairs-w8-M30", "out_pairs on the eight-wave form (9 k-steps x tile_c 8)", srcs=[(264, D)], cout=200, out_pairs=True, only=(lib.CONV_STREAM_LDS,), B=1, H=5, W=6)
# twin launches
_case("conv1", "twin-72to24", "the twin launch (blockIdx.y = 1) on the generic variant: 3 k-steps", srcs=[(72, D)], cout=24, twin=True, **_bhw(63))
_case("conv1", "twin-264to68", "the twin launch on the generic, LDS, DMA and split-K variants: 9 k-steps", srcs=[(264, D)], cout=68, twin=True, **_bhw(65))
_case("conv1", "twin-pool2", "the twin launch over pooled sources", srcs=[(72, POOL2)], cout=24, twin=True, B=2, H=3, W=5)
# the DMA ring (tile_k = 8: stages of two k-steps, four slots), split-K shares and the step ranges of CONV_STREAM_LDS
_DMA = [(pt, ct, lib.CONV_DMA) for pt in (1, 2) for ct in (4, 6, 8)]
for _ci, _st, _why in [(72, 3, "2 stages: fewer than the ring's four slots"), (136, 5, "3 stages (odd step count): fewer than ring slots"),
                       (256, 8, "8 steps: split-K gives each wave 2; 4 stages: one whole ring"),
                       (264, 9, "9 steps (odd): split-K shares 3 2 2 2; 5 stages: nstage % 4 = 1"), (296, 10, "10 steps: split-K shares 3 3 2 2; 5 stages"),
                       (328, 11, "11 steps (odd): split-K shares 3 3 3 2; 6 stages: nstage % 4 = 2"), (392, 13, "13 steps (odd): 7 stages: nstage % 4 = 3; the first wide CONV_STREAM_LDS form")]:
    _case("conv1", "steps%d" % _st, "VAR_DIRECT, " + _why, srcs=[(_ci, D)], cout=200, extra=_DMA, **_bhw(65 if _st % 2 else 17))
for _srcs, _st in [([(136, D), (40, UP2), (40, D)], 9), ([(200, D), (40, UP2), (40, D)], 11), ([(200, D), (72, UP2), (72, D)], 13), ([(40, D), (8, UP2)], 3)]:
    _case("conv1", "multi-steps%d" % _st, "VAR_MULTI on the DMA ring: %d steps" % _st, srcs=_srcs, cout=200, extra=_DMA, B=1, H=6, W=10)
for _ci, _st in [(376, 12), (616, 20), (744, 24), (808, 26)]:
    _case("conv1", "lds-steps%d" % _st, "CONV_STREAM_LDS at %d k-steps, an end of a range of stream_lds_ok (2 and 13: conv1-40to*, conv1-steps13); the last step partial" % _st,
          srcs=[(_ci, D)], cout=68, **_bhw(17))
# family B: the derived bound under SiLU and sigmoid
_case("conv1", "B-200to68", "the bound: 200 terms, SiLU", family="B", act=SILU, srcs=[(200, D)], cout=68, **_bhw(65))
_case("conv1", "B-sigmoid", "the bound under the sigmoid epilogue", family="B", act=SIGMOID, srcs=[(72, D)], cout=24, **_bhw(17))
_case("conv1", "B-multi3", "the bound over three sources", family="B", act=SILU, srcs=[(200, D), (40, UP2), (72, D)], cout=200, B=2, H=6, W=10)
_case("conv1", "B-pool2", "the bound over a pooled source", family="B", act=SILU, srcs=[(72, POOL2)], cout=68, B=2, H=3, W=5)
_case("conv1", "B-outf32", "the bound of an fp32 store", family="B", act=SIGMOID, srcs=[(264, D)], cout=68, out_f32=True, **_bhw(17))
_case("conv1", "B-f32", "the bound in fp32", family="B", dtype="f32", act=SILU, srcs=[(72, D)], cout=24, **_bhw(17))
_case("conv1", "B-twin", "the bound of both convs of a twin launch", family="B", act=SILU, srcs=[(264, D)], cout=68, twin=True, **_bhw(65))
_case("conv1", "B-pairs", "the bound of a pixel-pair store", family="B", act=SILU, srcs=[(72, D)], cout=24, out_pairs=True, only=(lib.CONV_STREAM_LDS,), B=2, H=3, W=6)

# --------------------------------------------------------------------------------------------------------------------------------------- OP_CONV3X3S2
_IN3 = [((1, 1), "a 1 x 1 input: the centre tap alone"), ((2, 2), "a 2 x 2 input, one output pixel: four taps"), ((3, 5), "3 x 5 (odd): the last tap column falls outside the map"),
        ((5, 4), "5 x 4: odd height, even width"), ((9, 13), "9 x 13: 5 x 7 outputs, more than one 16-pixel tile per image")]
for _i, ((_Hi, _Wi), _why) in enumerate(_IN3):
    for _j, _ci in enumerate((8, 24, 72)):
        _co = (24, 68)[(_i + _j) % 2]
        _case("conv3", "%dx%d-%dto%d" % (_Hi, _Wi, _ci, _co), "%s; %d k-steps (9 taps x %d)" % (_why, 9 * -(-_ci // 32), -(-_ci // 32)), srcs=[(_ci, D)], cout=_co, B=2, Hin=_Hi, Win=_Wi, extra=_DMA)
_case("conv3", "9x13-136to200", "45 k-steps: 23 DMA stages (nstage % 4 = 3), split-K shares 12 11 11 11", srcs=[(136, D)], cout=200, B=2, Hin=9, Win=13, extra=_DMA)
_case("conv3", "f32-3x5", "the fp32 instantiations", dtype="f32", srcs=[(24, D)], cout=24, B=2, Hin=3, Win=5)
_case("conv3", "f32-9x13", "the fp32 instantiations, several tiles", dtype="f32", srcs=[(8, D)], cout=68, B=2, Hin=9, Win=13)
for (_Hi, _Wi), _ci, _co in [((3, 5), 72, 24), ((9, 13), 24, 68), ((2, 2), 136, 200)]:
    _case("conv3", "twin-%dx%d-%dto%d" % (_Hi, _Wi, _ci, _co), "the twin launch on every variant that takes one", srcs=[(_ci, D)], cout=_co, twin=True, B=2, Hin=_Hi, Win=_Wi, extra=_DMA)
# CONV3_LDS (tile_k = 6): 4 x 16 output tiles, tile_c = workgroups / 64
_LDS3 = [(4, wg, lib.CONV3_LDS) for wg in (1, 4, 8, 12, 16)]
for _k, (_ci, _co) in enumerate([(48, 48), (48, 64), (64, 64)]):
    for _l, (_Hi, _Wi) in enumerate([(2, 2), (6, 10), (5, 7)]):
        _nc = _ci if _co == _ci and _Hi % 2 == 0 else 0
        _case("conv3", "lds-%dto%d-%dx%d" % (_ci, _co, _Hi, _Wi), "CONV3_LDS (weights and the patch of a 4 x 16 tile in LDS)%s" % (", with the pooled 1x1 branch %s the conv's slice" % ("behind", "in front of")[(_k + _l) % 2] if _nc else ""),
              srcs=[(_ci, D)], cout=_co, B=2, Hin=_Hi, Win=_Wi, nc=_nc, pool_front=bool((_k + _l) % 2), only=(lib.CONV3_LDS,), extra=_LDS3)
_case("conv3", "lds-second-unit", "CONV3_LDS on 64 workgroups over 70 tiles (2 x 5 x 7, ragged on both axes): some workgroups take a second tile", srcs=[(48, D)], cout=48, B=2, Hin=36, Win=200, nc=48,
      pool_front=True, only=(lib.CONV3_LDS,), extra=[(4, 1, lib.CONV3_LDS)])
# CONV3_WREG (tile_k = 7): 4 x 8 output tiles, tile_p = patch buffers, tile_c = workgroups per conv / 32
WREG_SHAPES = [(128, 128), (96, 96), (96, 64), (64, 64), (64, 96), (128, 96)]
_WREG = [(pt, wg, lib.CONV3_WREG) for wg in (2, 4, 8) for pt in (3, 2)]
for _k, (_ci, _co) in enumerate(WREG_SHAPES):
    _Hi, _Wi = [(2, 2), (6, 10), (5, 7)][_k % 3]
    _case("conv3", "wreg-%dto%d-%dx%d" % (_ci, _co, _Hi, _Wi), "CONV3_WREG on every workgroup count of the tuner, two and three patch buffers", srcs=[(_ci, D)], cout=_co, B=2, Hin=_Hi, Win=_Wi,
          only=(lib.CONV3_WREG,), extra=_WREG)
    _Hi, _Wi = [(5, 7), (2, 2), (6, 10)][_k % 3]
    _case("conv3", "wreg-twin-%dto%d-%dx%d" % (_ci, _co, _Hi, _Wi), "CONV3_WREG, twin launch", srcs=[(_ci, D)], cout=_co, twin=True, B=2, Hin=_Hi, Win=_Wi, only=(lib.CONV3_WREG,), extra=_WREG)
for _Hi, _Wi in [(2, 2), (6, 10)]:
    _case("conv3", "wreg-pool-%dx%d" % (_Hi, _Wi), "CONV3_WREG, the 96 -> 96 + 96 pooled branch", srcs=[(96, D)], cout=96, B=2, Hin=_Hi, Win=_Wi, nc=96, pool_front=True, only=(lib.CONV3_WREG,), extra=_WREG)
_case("conv3", "wreg-second-unit", "CONV3_WREG on 64 workgroups over 80 tiles (2 x 5 x 8, ragged on both axes): some workgroups take a second tile, with the pooled branch", srcs=[(96, D)], cout=96,
      B=2, Hin=36, Win=116, nc=96, pool_front=True, only=(lib.CONV3_WREG,), extra=[(3, 2, lib.CONV3_WREG), (2, 2, lib.CONV3_WREG)])
_case("conv3", "B-9x13-72to68", "the bound: 648 terms, SiLU", family="B", act=SILU, srcs=[(72, D)], cout=68, B=2, Hin=9, Win=13, extra=_DMA)
_case("conv3", "B-twin", "the bound of a twin launch", family="B", act=SILU, srcs=[(24, D)], cout=24, twin=True, B=2, Hin=5, Win=4)
_case("conv3", "B-f32", "the bound in fp32", family="B", dtype="f32", act=SILU, srcs=[(24, D)], cout=24, B=2, Hin=5, Win=4)
_case("conv3", "B-lds-pool", "the bound on CONV3_LDS with the pooled branch (SiLU hard-wired there)", family="B", act=SILU, srcs=[(64, D)], cout=64, B=2, Hin=6, Win=10, nc=64, pool_front=False, only=(lib.CONV3_LDS,), extra=_LDS3)
_case("conv3", "B-wreg-pool", "the bound on CONV3_WREG with the pooled branch", family="B", act=SILU, srcs=[(96, D)], cout=96, B=2, Hin=6, Win=10, nc=96, pool_front=True, only=(lib.CONV3_WREG,), extra=_WREG)

# ------------------------------------------------------------------------------------------------------------------------------------------- OP_DWCONV
DW_MAPS = list(_DW_MAPS) + [((3, 2), "W = 2: one pixel pair per row"), ((9, 11), "9 x 11: the matrix-core kernel's ragged map"), ((1, 1), "a single pixel: the centre tap alone"),
                            ((6, 20), "W = 20: even, no multiple of 8 or 16 tile columns")]
_seen = set()
for _i, _k in enumerate((3, 5, 7, 9)):
    for _j, ((_H, _W), _why) in enumerate(DW_MAPS):
        _C, _cw = _DW_C[(_i + _j) % 3]                       # 8, 24, 72
        _two = bool((_i + _j) % 2)
        _case("dw", "k%d-%dx%d-C%d%s" % (_k, _H, _W, _C, "-two" if _two else ""), "%s; C = %d: %s%s" % (_why, _C, _cw, "; Cout = 2 Cin" if _two else ""), act=NONE, B=2, H=_H, W=_W, C=_C, k=_k, two=_two)
for _i, _k in enumerate((3, 5, 7, 9)):                      # 2, 4 and 8 channel groups: what the staged-store form of the pixel-pair kernel needs (its waves divide Cin / 8)
    for _j, (_H, _W) in enumerate([(6, 20), (3, 2), (20, 20)]):
        _C = (16, 32, 64)[(_i + _j) % 3]
        _two = bool((_i + _j) % 2)
        _case("dw", "staged-k%d-%dx%d-C%d%s" % (_k, _H, _W, _C, "-two" if _two else ""), "%d channel groups: the staged stores of the pixel-pair kernel on 2%s waves" % (_C // 8, ", 4, 8"[:3 * (_C // 16).bit_length() - 3]),
              act=NONE, B=2, H=_H, W=_W, C=_C, k=_k, two=_two)
_case("dw", "B-staged", "the bound on the staged-store form", family="B", act=SILU, B=2, H=6, W=20, C=64, k=9, two=False)
_case("dw", "f32", "fp32: 4-channel groups (the generic kernel alone)", dtype="f32", act=NONE, B=2, H=9, W=13, C=12, k=5, two=False)
_case("dw", "f32-two", "fp32, Cout = 2 Cin", dtype="f32", act=NONE, B=2, H=4, W=4, C=12, k=7, two=True)
for _k, (_H, _W), _C, _two in [(3, (6, 20), 24, True), (5, (9, 11), 72, False), (7, (3, 2), 8, True), (9, (9, 13), 24, False), (9, (6, 20), 72, True), (5, (1, 1), 8, False)]:
    _case("dw", "B-k%d-%dx%d-C%d%s" % (_k, _H, _W, _C, "-two" if _two else ""), "the bound under SiLU: %d terms" % (_k * _k), family="B", act=SILU, B=2, H=_H, W=_W, C=_C, k=_k, two=_two)
_case("dw", "B-f32", "the bound in fp32", family="B", dtype="f32", act=SILU, B=2, H=4, W=4, C=12, k=7, two=False)

# ---------------------------------------------------------------------------------------------------------------------------------------------- OP_STEM
for _Hi, _Wi in [(2, 8), (6, 8), (10, 16)]:
    for _idt in ("f16", "f32", "u8"):
        for _dt in ("f16", "f32"):
            _case("stem", "%dx%d-%s-%s" % (_Hi, _Wi, _idt, _dt), "%s image, %s output; %s" % (_idt, _dt, "one output row" if _Hi == 2 else "W = 4: one quad per row" if _Wi == 8 else "two quads per row, 5 rows"),
                  family="B" if _idt == "u8" else "E", dtype=_dt, act=RELU, in_dtype=_idt, B=2, Hin=_Hi, Win=_Wi, cout=24 if _Hi != 6 else 8)

# ----------------------------------------------------------------------------------------------------------------------------------------- OP_SPPF_POOL
for (_H, _W), _B, _why in [((1, 1), 2, "a single pixel"), ((3, 64), 2, "W = 64: the widest map of the LDS kernel"), ((64, 64), 1, "64 x 64: the largest map of the LDS kernel"),
                           ((65, 5), 1, "H = 65: the fallback"), ((5, 65), 2, "W = 65: the fallback")]:
    _case("sppf", "%dx%d" % (_H, _W), _why + "; channel 3 holds -inf", family="E", act=NONE, B=_B, H=_H, W=_W, C=16)
_case("sppf", "f32-5x65", "fp32 on the fallback", family="E", dtype="f32", act=NONE, B=2, H=5, W=65, C=8)
_case("sppf", "f32-7x9", "fp32 on the LDS kernel", family="E", dtype="f32", act=NONE, B=2, H=7, W=9, C=8)

# ------------------------------------------------------------------------------------------------------------- OP_BOTTLENECK / OP_CONV1DW (family B: SiLU hard-wired)
_FMAPS = [((1, 1), "a single pixel"), ((15, 17), "15 x 17: one short of / one past the 16 x 16 tile"), ((17, 16), "17 x 16: a second tile row of one row")]
for _i, _c in enumerate((8, 32, 40, 64)):
    for _j, ((_H, _W), _why) in enumerate(_FMAPS):
        _k = (3, 5, 7, 9)[(_i + _j) % 4]
        _case("fused", "bneck-c%d-k%d-%dx%d" % (_c, _k, _H, _W), "OP_BOTTLENECK, c = %d (%s); %s" % (_c, "one k-step, tile_c 2 of the closing 1x1" if _c <= 32 else "two k-steps, tile_c 4", _why),
              family="B", act=SILU, sub="bneck", B=2, H=_H, W=_W, c=_c, k=_k, srcs=[(_c, D)])
TAILS = [(24, 3, 48, 2), (48, 5, 96, 2), (64, 5, 128, 2), (32, 3, 64, 3), (64, 5, 128, 3), (48, 3, 96, 3)]      # (c, k, C3, nsrc): the closing-conv instantiations
for _j, (_c, _k, _c3, _ns) in enumerate(TAILS):
    (_H, _W), _why = _FMAPS[1 + _j % 2]
    _case("fused", "tail-c%d-k%d-C%d-n%d" % (_c, _k, _c3, _ns), "OP_BOTTLENECK with the block's closing conv over %d slots + its own result; %s" % (_ns, _why),
          family="B", act=SILU, sub="tail", B=2, H=_H, W=_W, c=_c, k=_k, c3=_c3, srcs=[(_c, D)] * _ns)
for _i, _c in enumerate((8, 72, 192)):
    for _j, ((_H, _W), _why) in enumerate(_FMAPS):
        _k = (3, 5, 7, 9)[(_i + _j + 1) % 4]
        _case("fused", "c1dw-c%d-k%d-%dx%d" % (_c, _k, _H, _W), "OP_CONV1DW, c = %d: %d mid-channel blocks of 32%s; %s" % (_c, -(-3 * _c // 32), "" if 3 * _c % 32 == 0 else ", the last partial", _why),
              family="B", act=SILU, sub="c1dw", B=2, H=_H, W=_W, c=_c, k=_k, srcs=[(_c, D)])

# -------------------------------------------------------------------------------------------------------------------------------------------- OP_STEM2
# family E without the third conv on f16 / f32 images (both stages end in ReLU; integers of magnitude 1 keep the second stage's 9 C0 products of an LDS-resident
# fp16 integer <= 28 below 2048); family B on u8 images and with the third conv (SiLU)
STEM2_PAIRS = [(24, 48), (32, 64), (48, 96)]
for _third in (False, True):
    for _i, (_Hi, _Wi) in enumerate([(2, 8), (6, 8), (10, 12)]):
        for _j, _idt in enumerate(("f16", "f32", "u8")):
            _C0, _C1 = STEM2_PAIRS[(_i + _j) % 3]
            _rows, _split = (4, 8)[(_i + _j + _third) % 2], _third and bool((_i + _j) % 2)
            _case("stem2", "%dx%d-%s-%dto%d%s%s-rows%d" % (_Hi, _Wi, _idt, _C0, _C1, "-third" if _third else "", "-split" if _split else "", _rows),
                  "%s image %d x %d (%s), %d rows per tile%s%s" % (_idt, _Hi, _Wi, ("one output row", "3 x 4 at half resolution", "the twice-halved height is odd (10 -> 5 -> 3)")[_i], _rows,
                                                                  ", with the third conv" if _third else "", " and the split second output" if _split else ""),
                  family="B" if _third or _idt == "u8" else "E", act=RELU, in_dtype=_idt, B=2, Hin=_Hi, Win=_Wi, C0=_C0, cout=_C1, third=_third, split=_split, rows=_rows)

# ------------------------------------------------------------------------------------------------------------------------------------------- OP_HEADTAIL
HEAD_BEFORE, HEAD_AFTER = 37, 11                             # prediction rows of other levels around the level's own
_HM = {1: (1, 1, 1), 15: (1, 3, 5), 17: (1, 1, 17), 65: (1, 5, 13)}
for _i, _c in enumerate((64, 128, 192, 256, 384)):
    for _j, _M in enumerate((1, 15, 17, 65)):
        _it = (0, 1, 3)[(_i + _j) % 3]
        _B, _H, _W = _HM[_M] if (_i + _j) % 2 else (2,) + _HM[_M][1:]
        _case("head", "c%d-%dx%dx%d-iters%d" % (_c, _B, _H, _W, _it), "width %d (%s), %d pixels per image, %s units per wave, stride %d" % (
            _c, "weights LDS-resident" if _c <= 192 else "weights streamed", _H * _W, _it or "auto", (8, 16, 32)[_i % 3]),
              family="B", act=SILU, B=_B, H=_H, W=_W, c=_c, iters=_it, stride=(8, 16, 32)[_i % 3], srcs=[(_c, D), (_c, D)])

# ... and each with a c below the instantiation's maximum, where maf_bottleneck_tail_supported allows one (24 -> 48 on two slots is the 32-channel form: 16; the
# 64-channel forms: 40 and 56; 32 -> 64 on three slots: 8; 48 -> 96 on three slots: 40)
TAILS_BELOW = [(16, 3, 48, 2), (40, 5, 96, 2), (8, 3, 64, 3), (56, 5, 128, 3), (40, 3, 96, 3)]
for _j, (_c, _k, _c3, _ns) in enumerate(TAILS_BELOW):       # (at the end of the list: the seeds of the cases above stay what they were)
    (_H, _W), _why = _FMAPS[1 + _j % 2]
    _case("fused", "tail-c%d-k%d-C%d-n%d" % (_c, _k, _c3, _ns), "OP_BOTTLENECK with the closing conv, c = %d below the instantiation's maximum; %s" % (_c, _why),
          family="B", act=SILU, sub="tail", B=2, H=_H, W=_W, c=_c, k=_k, c3=_c3, srcs=[(_c, D)] * _ns)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(kind, pred=None):
    return [c["name"] for c in CASES if c["kind"] == kind and (pred is None or pred(c))]


def n_terms(c):
    """Products summed into one output element (the bias not counted)."""
    k = c["kind"]
    return sum(s[0] for s in c["srcs"]) * (9 if k == "conv3" else 1) if k in ("conv1", "conv3") else c["k"] ** 2 if k == "dw" else 27 if k in ("stem", "stem2") else 1


AMP = 3                                                        # |x|, |w|, |bias| <= 3 in family E


def _draw(c, shape, g, weight=False, scale=64):
    if c["family"] == "E":
        t = int_case(shape, g, amp=AMP, n_terms=n_terms(c))
    else:
        t = wide_case(shape, g)
        if weight:
            t = (t.float() / scale).half()                     # 2^-12 .. 1: the sums stay inside fp16's range
    return t.float() if weight or c["dtype"] == "f32" else t


def _bias(c, n, g):
    if c["family"] == "E":
        return torch.randint(-AMP, AMP + 1, (n,), generator=g).float() * (len(c["name"]) % 3 != 0)          # (a third of the cases: no bias)
    return torch.randn(n, generator=g)


def _conv_operands(c, g, k):
    cin, cout = sum(s[0] for s in c["srcs"]), c["cout"]
    if c["kind"] == "conv3":
        srcs = [_draw(c, (c["B"], c["Hin"], c["Win"], cin), g)]
    else:
        srcs = [_draw(c, (c["B"],) + src_grid(m, c["H"], c["W"]) + (C_,), g) for C_, m in c["srcs"]]
    return dict(srcs=srcs, w=_draw(c, (cout, cin, k, k), g, True), b=_bias(c, cout, g))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(c["seed"])
    kind = c["kind"]
    if kind in ("conv1", "conv3"):
        inp = _conv_operands(c, g, 3 if kind == "conv3" else 1)
        inp["twin"] = _conv_operands(c, g, 3 if kind == "conv3" else 1) if c.get("twin") else None
        if c.get("nc"):
            inp["pool1"] = (_draw(c, (c["nc"], c["srcs"][0][0], 1, 1), g, True), _bias(c, c["nc"], g))
        return inp
    if kind == "dw":
        cout = c["C"] * (2 if c["two"] else 1)
        return dict(srcs=[_draw(c, (c["B"], c["H"], c["W"], c["C"]), g)], w=_draw(c, (cout, 1, c["k"], c["k"]), g, True), b=_bias(c, cout, g))
    if kind == "stem":
        shape = (c["B"], 3, c["Hin"], c["Win"])
        if c["in_dtype"] == "u8":
            img = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
            w = torch.randn(c["cout"], 3, 3, 3, generator=g) / 5.0
        else:
            img = torch.randint(-AMP, AMP + 1, shape, generator=g).to(torch.float16 if c["in_dtype"] == "f16" else torch.float32)
            w = torch.randint(-AMP, AMP + 1, (c["cout"], 3, 3, 3), generator=g).float()
        return dict(image=img, w=w, b=_bias(c, c["cout"], g), srcs=[])
    if kind == "stem2":
        shape, C0, C1 = (c["B"], 3, c["Hin"], c["Win"]), c["C0"], c["cout"]
        if c["family"] == "E":                                 # integers of magnitude 1
            img = torch.randint(-1, 2, shape, generator=g).to(torch.float16 if c["in_dtype"] == "f16" else torch.float32)
            raw = [torch.randint(-1, 2, (C0, 3, 3, 3), generator=g).float(), torch.randint(-1, 2, (C0,), generator=g).float(),
                   torch.randint(-1, 2, (C1, C0, 3, 3), generator=g).float(), torch.randint(-1, 2, (C1,), generator=g).float()]
        else:
            img = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if c["in_dtype"] == "u8" else wide_case(shape, g).to(torch.float16 if c["in_dtype"] == "f16" else torch.float32)
            raw = [(torch.randn(C0, 3, 3, 3, generator=g) / 27 ** 0.5 * 2).half().float(), torch.randn(C0, generator=g) * 0.2,
                   (torch.randn(C1, C0, 3, 3, generator=g) / (9 * C0) ** 0.5 * 2).half().float(), torch.randn(C1, generator=g) * 0.2]
        if c["third"]:
            raw += [(torch.randn(C1, C1, 1, 1, generator=g) / C1 ** 0.5 * 2).half().float(), torch.randn(C1, generator=g) * 0.2]
        return dict(image=img, w=raw[0], raw=raw, srcs=[])
    if kind == "head":
        cc = c["c"]
        raw = []
        for n, sc, sh in ((80, 2.0, -2.0), (68, 2.0, 0.0)):       # cls_conv_s + cls_pred, reg_conv_s + reg_pred (the scales of test_gpu_fused_parity.py)
            raw += [(torch.randn(cc, cc, 1, 1, generator=g) / cc ** 0.5).half().float(), torch.randn(cc, generator=g) * 0.3,
                    (torch.randn(n, cc, 1, 1, generator=g) * (sc / cc ** 0.5)).half().float(), torch.randn(n, generator=g) * 0.5 + sh]
        # wide_case / 16 (exact in fp16 but for its subnormals): binades 2^-10 .. 2^2, so that the logits do not saturate the sigmoid and the softmax
        return dict(srcs=[(wide_case((c["B"], c["H"], c["W"], cc), g).float() / 16).half() for _ in range(2)], raw=raw)
    if kind == "fused":
        cc, k, mid, ns = c["c"], c["k"], 3 * c["c"], len(c["srcs"])

        def wt(*shape):
            fan = shape[1] * shape[2] * shape[3] if shape[1] > 1 else shape[2]
            return (torch.randn(*shape, generator=g) / fan ** 0.5).half().float()
        raw = [wt(mid, cc, 1, 1), torch.randn(mid, generator=g) * 0.3, None, torch.randn(mid, generator=g) * 0.3]
        if c["sub"] != "c1dw":
            raw += [wt(cc, mid, 1, 1), torch.randn(cc, generator=g) * 0.3]
        if c["sub"] == "tail":
            raw += [wt(c["c3"], (ns + 1) * cc, 1, 1), torch.randn(c["c3"], generator=g) * 0.3]
        # srcs[0]: the bottleneck's input (the LAST concat slot), srcs[1:]: the slots in front of it, in order
        return dict(srcs=[wide_case((c["B"], c["H"], c["W"], cc), g) for _ in range(ns)], w=wt(mid, 1, k, k), raw=raw)
    assert kind == "sppf"
    x = wide_case((c["B"], c["H"], c["W"], c["C"]), g)
    x[..., 3] = float("-inf")
    x[0, c["H"] // 2, c["W"] // 2, 3] = 1.0                    # ... but for one pixel, whose 5 x 5, 9 x 9 and 13 x 13 neighbourhoods must pick it up
    return dict(srcs=[x.float() if c["dtype"] == "f32" else x])


def inputs(case):
    """{"srcs": [NHWC source per concat slot, the case's dtype], "w", "b" (fp32 holding fp16 values), "twin": the second conv's, "pool1": (w1, b1), "image"} on the
    CPU.  Shared: do not write to them."""
    return _inputs(case["name"])


def out_grid(c):
    if c["kind"] == "stem2":
        return ((c["Hin"] - 1) // 2) // 2 + 1, ((c["Win"] - 1) // 2) // 2 + 1
    if c["kind"] in ("conv3", "stem"):
        return (c["Hin"] - 1) // 2 + 1, (c["Win"] - 1) // 2 + 1
    return c["H"], c["W"]


_DT = {"f16": lib.F16, "f32": lib.F32, "u8": lib.U8}
_KIND = {"fused": lib.OP_BOTTLENECK, "conv1": lib.OP_CONV1X1, "conv3": lib.OP_CONV3X3S2, "dw": lib.OP_DWCONV, "stem": lib.OP_STEM, "sppf": lib.OP_SPPF_POOL}


def _fake_op(c, modes):
    H, W = out_grid(c)
    cout = c.get("cout", c.get("C", 0) * (2 if c.get("two") else 1))
    if c["kind"] == "stem2":
        return NS(kind=lib.OP_STEM2, dtype=lib.F16, in_dtype=_DT[c["in_dtype"]], act=RELU, B=c["B"], H=H, W=W, Hin=c["Hin"], Win=c["Win"], Cout=c["cout"], out_f32=0,
                  nc=c["cout"] if c["third"] else 0, aux=[int(c["split"])], src=[])
    if c["kind"] == "head":
        return NS(kind=lib.OP_HEADTAIL, dtype=lib.F16, in_dtype=lib.F16, act=SILU, B=c["B"], H=H, W=W, Cout=85, out_f32=1, nc=80, reg_max=16, lvl_stride=[float(c["stride"])],
                  src=[NS(mode=D), NS(mode=D)])
    if c["kind"] == "fused":
        return NS(kind=lib.OP_CONV1DW if c["sub"] == "c1dw" else lib.OP_BOTTLENECK, dtype=lib.F16, in_dtype=lib.F16, act=SILU, B=c["B"], H=H, W=W, Cout=c["c"], out_f32=0,
                  nc=c.get("c3", 0), src=[NS(mode=D) for _ in c["srcs"]])
    return NS(kind=_KIND[c["kind"]], dtype=_DT[c["dtype"]], in_dtype=_DT[c.get("in_dtype", c["dtype"])], act=c["act"], B=c["B"], H=H, W=W, Hin=c.get("Hin", 0), Win=c.get("Win", 0),
              Cout=cout, out_f32=int(bool(c.get("out_f32"))), nc=c.get("nc", 0), src=[NS(mode=m) for m in modes])


def _ksteps_lo(C_, dtype):
    """First channel of the last (possibly partial) k-step of a source of C_ channels; a source of one k-step: its last 16-byte chunk."""
    ks = 32 if dtype == "f16" else 16
    lo = (C_ - 1) // ks * ks
    return lo if lo > 0 else C_ - ks // 4


def mutate(c, inp, mut):
    """(inputs, source modes) of `c` damaged as a wrong kernel would read them.  tap: the centre tap of the filter dropped (the one tap every output pixel of every map has); kstep: the last k-step's channels of every
    source dropped (depth-wise, SPPF: the last 16-byte channel group); row / col: the last row / column of every source dropped; batch: the images swapped; up2: the
    up-sampled sources read at the wrong parity (pixel (x + 1) >> 1); pool2: the window's first element instead of its maximum; chunk: the last 16-byte channel chunk of
    source 0 read from chunk 0 (a neighbouring chunk in place of the slice's own); div255: the u8 image not divided by 255."""
    kind = c["kind"]
    modes = [s[1] for s in c["srcs"]] if kind in ("conv1", "fused", "head") else [D]
    H, W = out_grid(c)
    ch = 8 if c["dtype"] == "f16" else 4

    def one(o):
        o = dict(o)
        srcs = [s.clone() for s in o["srcs"]]
        if mut == "tap":
            o["w"] = o["w"].clone()
            o["w"][..., o["w"].shape[-2] // 2, o["w"].shape[-1] // 2] = 0
        elif mut == "kstep":
            for s in srcs:
                s[..., (_ksteps_lo(s.shape[-1], c["dtype"]) if kind in ("conv1", "conv3", "fused", "head") else s.shape[-1] - ch):] = 0 if kind != "sppf" else float("-inf")
        elif mut == "row":                                     # (a SUB2 source: the last row it reads, the last but one)
            for s, m in zip(srcs, modes):
                s[:, -2 if m == SUB2 else -1] = 0 if kind != "sppf" else float("-inf")
        elif mut == "col":
            for s, m in zip(srcs, modes):
                s[:, :, -2 if m == SUB2 else -1] = 0 if kind != "sppf" else float("-inf")
        elif mut == "batch":
            srcs = [s.flip(0) for s in srcs]
        elif mut == "chunk":
            srcs[0][..., -ch:] = srcs[0][..., :ch]
        elif mut == "up2":
            for i, m in enumerate(modes):
                if m == UP2:
                    srcs[i] = srcs[i].repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].roll(-1, 2)
        elif mut not in ("pool2", "div255"):
            raise ValueError(mut)
        if "image" in o and mut in ("row", "col", "batch", "div255"):
            img = o["image"].clone()
            if mut == "row":
                img[:, :, -1] = 0
            elif mut == "col":
                img[..., -1] = 0
            elif mut == "batch":
                img = img.flip(0)
            else:
                img = img.float() * 255.0                      # (the reference divides by 255: as if the kernel had not)
            o["image"] = img
        o["srcs"] = srcs
        return o

    out = one(inp)
    if inp.get("twin"):
        out["twin"] = one(inp["twin"])
    if mut == "up2":
        modes = [D if m == UP2 else m for m in modes]
    if mut == "pool2":
        modes = [SUB2 if m == POOL2 else m for m in modes]
    return out, modes


def reference(case, inp=None, mut=None):
    """{output name: (ref float64 NHWC, bound, S)} of `case` on `inp` (default: its own inputs), through op_ref.reference.  Outputs: "out"; "twin" (the second conv of a
    twin launch); "pool" (the pooled 1x1 branch of CONV3_LDS / CONV3_WREG)."""
    c = case
    inp = inputs(c) if inp is None else inp
    modes = [s[1] for s in c["srcs"]] if c["kind"] in ("conv1", "fused", "head") else [D]
    if mut is not None:
        inp, modes = mutate(c, inp, mut)
    op = _fake_op(c, modes)
    cpu = torch.device("cpu")
    if c["kind"] == "conv3":
        rec = dict(raw=[inp["w"], inp["b"]])
        if c.get("nc"):
            rec["pool1"] = inp["pool1"]
        if inp.get("twin"):
            rec["twin"] = dict(raw=(inp["twin"]["w"], inp["twin"]["b"]))
        return op_ref.reference(op, rec, inp["srcs"], cpu, twin_src=inp["twin"]["srcs"][0] if inp.get("twin") else None)
    if c["kind"] == "stem":
        return op_ref.reference(op, dict(raw=[inp["w"], inp["b"]]), [], cpu, image=inp["image"])
    if c["kind"] == "stem2":
        return op_ref.reference(op, dict(raw=[inp["w"]] + inp["raw"][1:]), [], cpu, image=inp["image"])
    if c["kind"] == "sppf":
        return op_ref.reference(op, dict(raw=[]), inp["srcs"], cpu)
    if c["kind"] == "head":
        return op_ref.reference(op, dict(raw=inp["raw"]), inp["srcs"], cpu)
    if c["kind"] == "fused":
        return op_ref.reference(op, dict(raw=inp["raw"][:2] + [inp["w"]] + inp["raw"][3:]), inp["srcs"], cpu)
    out = op_ref.reference(op, dict(raw=[inp["w"], inp["b"]]), inp["srcs"], cpu)
    if inp.get("twin"):
        out["twin"] = op_ref.reference(op, dict(raw=[inp["twin"]["w"], inp["twin"]["b"]]), inp["twin"]["srcs"], cpu)["out"]
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    return reference(BY_NAME[name])


def case_reference(case):
    """reference(case) on its own inputs, computed once per process.  Shared: do not write to it."""
    return _reference(case["name"])


def is_exact(c, key):
    """Whether output `key` of the case is checked bit for bit: family E, but for the pooled 1x1 branch of the 3x3 stride-2 kernels (its SiLU is hard-wired: the
    bound) — and SPPF, whose max-pools move values unchanged."""
    return c["family"] == "E" and key != "pool"


def store_dtype(c):
    return torch.float32 if c["dtype"] == "f32" or c.get("out_f32") else torch.float16
