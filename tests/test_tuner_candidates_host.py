"""Host side of the tuners' candidate lists (tuner.candidates / conv_tiles / dw_tiles, train_ops.conv_candidates) on hand-built MafOp structs: no
duplicates, the 48 -> 96 stem offers the one tile height its kernel takes, the DMA ring (tile_k = 8) only where its kernel is meant to run, and the
training enumerator's list for the shapes test_gpu_train.py runs."""
from types import SimpleNamespace

import pytest
import torch

from maf_yolo_amd import conv_variants, lib, pack, train_ops, tuner


def _op(kind, B, H, W, cin, cout, srcs=None, ksize=0, out_stride=None, out_f32=0, act=lib.ACT_SILU):
    o = lib.MafOp()
    o.kind, o.dtype, o.in_dtype, o.act = kind, lib.F16, lib.F16, act
    o.B, o.H, o.W, o.Cin, o.Cout, o.ksize = B, H, W, cin, cout, ksize
    srcs = srcs or [(cin, lib.SRC_DIRECT)]
    o.nsrc = len(srcs)
    for k, (c, mode) in enumerate(srcs):
        o.src[k].C, o.src[k].stride, o.src[k].mode = c, c, mode
    o.out_stride, o.out_f32 = out_stride or cout, out_f32
    return o


def _plan(ops, recs, B):
    return SimpleNamespace(ops=ops, _ops=recs, dtype=lib.F16, B=B, device="cpu", _pairs_producer=lambda i: None)


def _conv_plan(kind, B, H, W, cin, cout, **kw):
    o = _op(kind, B, H, W, cin, cout, **kw)
    srcC = [o.src[k].C for k in range(o.nsrc)]
    w = torch.randn(cout, cin, *((3, 3) if kind == lib.OP_CONV3X3S2 else (1, 1)))
    return _plan([o], [dict(raw=(w, torch.randn(cout), srcC if kind == lib.OP_CONV1X1 else None))], B)


_CONVS = [(lib.OP_CONV1X1, 32, 160, 160, 48, 48), (lib.OP_CONV1X1, 32, 20, 20, 288, 96), (lib.OP_CONV1X1, 1, 20, 20, 1280, 640),
          (lib.OP_CONV1X1, 32, 40, 40, 640, 192), (lib.OP_CONV1X1, 3, 11, 19, 448, 128), (lib.OP_CONV3X3S2, 32, 80, 80, 48, 64),
          (lib.OP_CONV3X3S2, 32, 40, 40, 96, 96), (lib.OP_CONV3X3S2, 1, 10, 10, 384, 384), (lib.OP_CONV1X1, 32, 80, 80, 256, 68)]


@pytest.mark.parametrize("kind,B,H,W,cin,cout", _CONVS)
def test_conv_candidates_are_distinct_and_the_dma_ring_only_where_meant(kind, B, H, W, cin, cout):
    plan = _conv_plan(kind, B, H, W, cin, cout)
    cands = tuner.candidates(plan, 0)
    tiles = [c_.tiles for c_ in cands]
    assert tiles == tuner.conv_tiles(plan, 0) and len(set(tiles)) == len(tiles) and tiles
    ksteps = -(-cin // 32) * (9 if kind == lib.OP_CONV3X3S2 else 1)
    for pt, ct, tk in tiles:
        if tk == 8:
            assert pt <= 2 and ksteps >= 8 and ct >= 4
    for c_ in cands:                                                      # each candidate carries its own packing
        assert c_.op.w == c_.keep[0].data_ptr() and c_.op.bias == c_.keep[1].data_ptr() and c_.op.out_pairs == 0
        assert (c_.op.tile_p, c_.op.tile_c, c_.op.tile_k) == c_.tiles


def test_conv_candidates_with_multiple_sources_and_pooling():
    plan = _conv_plan(lib.OP_CONV1X1, 32, 40, 40, 384, 128, srcs=[(128, lib.SRC_UP2), (256, lib.SRC_DIRECT)])
    tiles = tuner.conv_tiles(plan, 0)
    assert len(set(tiles)) == len(tiles) and not any(t[2] == 3 for t in tiles)      # the stream form needs one direct source
    plan = _conv_plan(lib.OP_CONV1X1, 32, 80, 80, 64, 64, srcs=[(64, lib.SRC_POOL2)])
    tiles = tuner.conv_tiles(plan, 0)
    assert not any(t[2] in (2, 8) for t in tiles)                                   # no LDS-shared fragments behind a pooled source


@pytest.mark.parametrize("cout,c0,rows", [(48, 24, (8, 4)), (64, 32, (8, 4)), (96, 48, (4,))])
def test_stem2_candidates(cout, c0, rows):
    o = _op(lib.OP_STEM2, 32, 160, 160, 3, cout, ksize=c0, act=lib.ACT_RELU)
    tiles = [c_.tiles for c_ in tuner.candidates(_plan([o], [{}], 32), 0)]
    assert len(set(tiles)) == len(tiles)
    assert sorted({t[0] for t in tiles}) == sorted(rows) and {t[2] for t in tiles} == {256, 512, 768, 1024}


def test_head_tail_and_depthwise_candidates_are_distinct():
    o = _op(lib.OP_HEADTAIL, 32, 80, 80, 128, 85)
    assert [c_.tiles for c_ in tuner.candidates(_plan([o], [{}], 32), 0)] == [(0, 0, i) for i in (1, 2, 3, 4, 6)]
    for H, W, C_, k, cout in ((20, 20, 576, 9, 576), (80, 80, 128, 3, 256), (11, 19, 192, 5, 192), (160, 160, 48, 5, 48)):
        o = _op(lib.OP_DWCONV, 32, H, W, C_, cout, ksize=k, act=lib.ACT_NONE)
        o.aux[0] = 1                                                       # (a matrix-core operand exists)
        cands = tuner.candidates(_plan([o], [{}], 32), 0)
        tiles = [c_.tiles for c_ in cands]
        assert len(set(tiles)) == len(tiles) and (-1, 0, 0) in tiles and any(t[0] == -2 for t in tiles)
        assert not any(c_.pairs for c_ in cands)                          # no pair producer: no pixel-pair variant
        assert all(c_.op.src[0].mode == lib.SRC_DIRECT for c_ in cands)


# the 14 shapes of test_gpu_train.py::test_every_conv_variant_the_train_tuner_may_pick
_TRAIN = [((8, 40, 40), 64, 192), ((4, 80, 80), 192, 64), ((8, 20, 20), 288, 96), ((2, 160, 160), 24, 72), ((2, 4, 4), 576, 384), ((2, 4, 4), 768, 384),
          ((2, 8, 8), 448, 128), ((2, 4, 4), 96, 288), ((2, 16, 16), 288, 128), ((2, 4, 4), 480, 192), ((1, 3, 5), 640, 256), ((2, 16, 16), 48, 48),
          ((2, 8, 8), 128, 80), ((2, 4, 4), 192, 68)]


@pytest.mark.parametrize("M_hw,cin,cout", _TRAIN)
def test_train_enumerator(M_hw, cin, cout):
    M = M_hw[0] * M_hw[1] * M_hw[2]
    cands = train_ops.conv_candidates(M, cin, cout)
    ksteps = -(-cin // 32)
    assert len(set(cands)) == len(cands) >= 6
    assert (*pack.tile_for(cout, M), 1) in cands                           # the static rule's tile is always timed
    for pt, ct, tk in cands:
        assert tk in (1, 2, 3, 4, 5, 8) and ct in (2, 4, 6, 8) and pt in (1, 2, 4)
        if tk == 8:
            assert pt <= 2 and ksteps >= 8 and ct >= 4
        if (pt, tk) == (2, 5):
            assert ct >= 4 and 64 <= ksteps * ct <= 160
    if ksteps >= 8:
        assert any(c_[2] == 8 for c_ in cands)


# the lists as _conv_choice timed them before conv_candidates existed (same code, moved): any drop, addition or reordering shows here
_TRAIN_LISTS = {
    (12800, 64, 192): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 3), (2, 2, 3), (1, 2, 5), (1, 4, 1), (2, 4, 1), (1, 4, 3), (2, 4, 3), (1, 4, 5), (1, 6, 1), (1, 6, 3), (2, 6, 3), (1, 6, 5), (1, 8, 1), (1, 8, 3), (2, 8, 3), (1, 8, 5)],
    (25600, 192, 64): [(1, 2, 1), (2, 2, 1), (1, 2, 5), (1, 4, 1), (1, 4, 5), (1, 4, 2), (1, 6, 1), (1, 6, 5), (1, 6, 2), (1, 8, 1), (1, 8, 5), (1, 8, 2)],
    (3200, 288, 96): [(1, 2, 1), (1, 2, 4), (1, 2, 5), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (51200, 24, 72): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 3), (2, 2, 3), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 3), (2, 4, 3), (1, 6, 1), (2, 6, 1), (1, 6, 3), (2, 6, 3), (1, 8, 1), (2, 8, 1), (1, 8, 3), (2, 8, 3)],
    (32, 576, 384): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (2, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (32, 768, 384): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (2, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
    (128, 448, 128): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (32, 96, 288): [(1, 2, 1), (1, 2, 3), (2, 2, 3), (1, 2, 5), (1, 4, 1), (1, 4, 3), (2, 4, 3), (1, 4, 5), (1, 6, 1), (1, 6, 5), (1, 8, 1), (1, 8, 5)],
    (512, 288, 128): [(1, 2, 1), (1, 2, 4), (1, 2, 5), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (32, 480, 192): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (15, 640, 256): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (2, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (512, 48, 48): [(1, 2, 1), (1, 2, 3), (2, 2, 3), (1, 2, 5), (1, 4, 1), (1, 4, 3), (2, 4, 3), (1, 4, 5), (1, 6, 1), (1, 6, 3), (2, 6, 3), (1, 6, 5)],
    (128, 128, 80): [(1, 2, 1), (1, 2, 3), (2, 2, 3), (1, 2, 5), (1, 4, 1), (1, 4, 3), (2, 4, 3), (1, 4, 5), (1, 4, 2), (1, 6, 1), (1, 6, 5), (1, 6, 2), (1, 8, 1), (1, 8, 5), (1, 8, 2)],
    (32, 192, 68): [(1, 2, 1), (1, 2, 5), (1, 4, 1), (1, 4, 5), (1, 4, 2), (1, 6, 1), (1, 6, 5), (1, 6, 2)],
}


def test_train_enumerator_lists_are_pinned():
    for (M, K, N), want in _TRAIN_LISTS.items():
        assert train_ops.conv_candidates(M, K, N) == want, (M, K, N)


# tuner.conv_tiles for _CONVS, keyed like them, as the commit before conv_variants.py returned them (three enumerators, one per tuner): whole lists, order included
_INFER_LISTS = {
    (1, 32, 160, 160, 48, 48): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 3), (2, 2, 3), (1, 2, 5), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 3), (2, 4, 3), (1, 4, 5), (1, 6, 1), (2, 6, 1), (1, 6, 3), (2, 6, 3), (1, 6, 5)],
    (1, 32, 20, 20, 288, 96): [(1, 2, 1), (2, 2, 1), (1, 2, 4), (1, 2, 5), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (1, 1, 20, 20, 1280, 640): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
    (1, 32, 40, 40, 640, 192): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 4), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 4), (1, 4, 5), (2, 4, 5), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
    (1, 3, 11, 19, 448, 128): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8)],
    (2, 32, 80, 80, 48, 64): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 4, 1), (2, 4, 1), (4, 4, 1), (4, 4, 6), (4, 8, 6), (4, 12, 6), (4, 16, 6), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
    (2, 32, 40, 40, 96, 96): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 4), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 4), (3, 2, 7), (2, 2, 7), (3, 4, 7), (2, 4, 7), (3, 8, 7), (2, 8, 7), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
    (2, 1, 10, 10, 384, 384): [(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
    (1, 32, 80, 80, 256, 68): [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 5), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 5), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 5), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8)],
}
# ... for the two cases of test_conv_candidates_with_multiple_sources_and_pooling, a twin launch, MPRep in one launch on either 3x3 kernel and an fp32 plan
_INFER_SPECIAL = {
    'up2+direct': [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 4), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 4), (1, 4, 5), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 4), (1, 6, 5), (2, 6, 5), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 4), (1, 8, 5), (2, 8, 5), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
    'pooled': [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 5), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 5), (1, 6, 1), (2, 6, 1), (1, 6, 5), (1, 8, 1), (2, 8, 1), (1, 8, 5)],
    'twin': [(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 2), (2, 4, 2), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 2), (2, 6, 2), (1, 8, 1), (2, 8, 1), (1, 8, 2), (2, 8, 2)],
    'pool1_tk6': [(4, 4, 6), (4, 8, 6), (4, 12, 6), (4, 16, 6)],
    'pool1_tk7': [(3, 2, 7), (2, 2, 7), (3, 4, 7), (2, 4, 7), (3, 8, 7), (2, 8, 7)],
    'fp32': [(1, 2, 1), (1, 4, 1), (1, 6, 1), (1, 8, 1)],
}
# (M, cin, cout) -> (forward list, data-gradient list) of the training 3x3 stride-2 tuner, from the same commit
_TRAIN3_LISTS = {
    (204800, 48, 64): ([(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
        [(1, 2, 0), (2, 2, 0), (4, 2, 0), (1, 4, 0), (2, 4, 0), (4, 4, 0)]),
    (51200, 96, 96): ([(1, 2, 1), (2, 2, 1), (4, 2, 1), (1, 2, 4), (1, 4, 1), (2, 4, 1), (4, 4, 1), (1, 4, 4), (1, 4, 2), (1, 4, 8), (2, 4, 2), (2, 4, 8), (4, 4, 2), (1, 6, 1), (2, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (2, 6, 2), (2, 6, 8), (1, 8, 1), (2, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8), (2, 8, 2), (2, 8, 8)],
        [(1, 2, 0), (2, 2, 0), (4, 2, 0), (1, 4, 0), (2, 4, 0), (1, 8, 0)]),
    (100, 384, 384): ([(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
        [(1, 2, 0), (1, 4, 0), (1, 8, 0)]),
    (3200, 128, 128): ([(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
        [(1, 2, 0), (1, 4, 0), (1, 8, 0)]),
    (128, 64, 64): ([(1, 2, 1), (1, 2, 4), (1, 4, 1), (1, 4, 4), (1, 4, 2), (1, 4, 8), (1, 6, 1), (1, 6, 4), (1, 6, 2), (1, 6, 8), (1, 8, 1), (1, 8, 4), (1, 8, 2), (1, 8, 8)],
        [(1, 2, 0), (1, 4, 0), (1, 8, 0)]),
}


@pytest.mark.parametrize("conv", _CONVS)
def test_inference_enumerator_lists_are_pinned(conv):
    assert tuner.conv_tiles(_conv_plan(*conv), 0) == _INFER_LISTS[conv]


def _special_plan(kind, B, H, W, cin, cout, rec=None, dtype=lib.F16, **kw):
    plan = _conv_plan(kind, B, H, W, cin, cout, **kw)
    plan._ops[0].update(rec or {})
    plan.dtype = plan.ops[0].dtype = dtype
    return plan


def test_inference_enumerator_special_lists_are_pinned():
    plans = {
        "up2+direct": _special_plan(lib.OP_CONV1X1, 32, 40, 40, 384, 128, srcs=[(128, lib.SRC_UP2), (256, lib.SRC_DIRECT)]),
        "pooled": _special_plan(lib.OP_CONV1X1, 32, 80, 80, 64, 64, srcs=[(64, lib.SRC_POOL2)]),
        "twin": _special_plan(lib.OP_CONV1X1, 32, 40, 40, 128, 128, rec=dict(twin=dict(raw=None))),
        "pool1_tk6": _special_plan(lib.OP_CONV3X3S2, 32, 80, 80, 48, 48, rec=dict(pool1=(1,), pool1_tk=lib.CONV3_LDS)),
        "pool1_tk7": _special_plan(lib.OP_CONV3X3S2, 32, 80, 80, 96, 96, rec=dict(pool1=(1,), pool1_tk=lib.CONV3_WREG)),
        "fp32": _special_plan(lib.OP_CONV1X1, 1, 20, 20, 64, 64, dtype=lib.F32),
    }
    assert set(plans) == set(_INFER_SPECIAL)
    for name, plan in plans.items():
        assert tuner.conv_tiles(plan, 0) == _INFER_SPECIAL[name], name
    assert {t[2] for t in _INFER_SPECIAL["fp32"]} <= {lib.CONV_GENERIC, lib.CONV_SPLITK}
    assert {t[2] for t in _INFER_SPECIAL["twin"]} <= {lib.CONV_GENERIC, lib.CONV_LDS, lib.CONV_SPLITK, lib.CONV3_WREG, lib.CONV_DMA}


@pytest.mark.parametrize("M,cin,cout", list(_TRAIN3_LISTS))
def test_train_3x3_enumerator_lists_are_pinned(M, cin, cout):
    fwd, dgrad = _TRAIN3_LISTS[(M, cin, cout)]
    assert train_ops._conv3_fwd_cands(cin, cout, M, (*pack.tile_for(cout, M), lib.CONV_GENERIC)) == fwd
    assert conv_variants.conv3_dgrad_tiles(cin, M, (*train_ops._tile_dgrad(cin, M), 0)) == dgrad
    # the forward list is the inference tuner's for the same op, without the kernels whose record holds a bias, and the static tile
    infer = [t for t in tuner.conv_tiles(_conv_plan(lib.OP_CONV3X3S2, 1, 1, M, cin, cout), 0) if t[2] not in (lib.CONV3_LDS, lib.CONV3_WREG)]
    assert fwd[:len(infer)] == infer and len(fwd) - len(infer) <= 1
