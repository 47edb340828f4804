"""-m gpu: every producer of training-mode BatchNorm batch statistics against an fp64 reference (tests/bn_ref.py).

The variance of csrc/bn_act.hip is one-pass: the producers accumulate {sum x, sum x^2} in fp32 (lane sums, wave shuffles, LDS atomics, global atomics into up to 16
replicas), bn_apply_kernel folds the replicas in double and takes var = q/M - (s/M)^2, which loses digits as |mean| / std of what was summed grows (bn_act's own
statistics launch takes the sum of squares about a per-channel pivot — the median of three of the tensor's pixels — for that reason; the other producers hand over raw sums).  Four kernels produce the sums for the
same apply pass (bn_stats_kernel, the 1x1 conv's epilogue, the depth-wise branches' epilogue, the STATS form of csrc/bn_sum.hip) and all share one scratch protocol
(two halves, alternating phase, replica count min(R, 16, 1024 / C) inside one buffer per stream and ceil(C / 256)).  The other BatchNorm tests compare with the
framework's fp32 result at |mean| / std ~ 0.25, or one producer with another: a loss of accuracy common to all producers, or a stale replica, passes them.

Here EVERY comparison is against fp64 on the stored values the kernel read: no case compares one kernel path with another.
Errors: max |got - ref| / max |ref| per tensor (y, dx, dgamma, dbeta, save_mean, running_mean); relative per channel for save_rstd and running_var.
Bars (bn_ref.BARS: those of test_gpu_train.py::test_bn_act_forward_backward): fp32 2e-4 for y, 4e-4 for the gradients, 1e-4 for the statistics; fp16 storage 1e-2,
2e-2 and 2e-3 (the fp16 reference rounds y / dx to fp16 last).  The rung with |mean| / std = 64 is held to 10 x those bars: a gross-error condition; what the kernels
measure there is in DESIGN.md (BatchNorm section)."""
import ctypes as C

import pytest
import torch

from maf_yolo_amd import lib, tape as tape_mod, train_ops

import bn_ref
from bn_ref import as_nchw, bn_ref as ref64, err_max, err_rel, ladder_rows, moments, rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS, MOM = 1e-3, 0.03
F16, F32 = torch.float16, torch.float32
DTN = {F16: "fp16", F32: "fp32"}


def _bn(c, g, gamma=None):
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5 if gamma is None else torch.full((c,), float(gamma)))
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    return bn.to(DEV).train()


def _check(got, ref, dtype, tag, mult=1):
    """every tensor of `got` against its fp64 reference at the bar of its kind; prints each figure, then asserts all of them"""
    bar = bn_ref.BARS[dtype]
    kinds = dict(y=("y", err_max), dx=("grad", err_max), dres=("grad", err_max), dgamma=("grad", err_max), dbeta=("grad", err_max),
                 mean=("stat", err_max), running_mean=("stat", err_max), rstd=("stat", err_rel), running_var=("stat", err_rel))
    bad, line = [], []
    for name, t in got.items():
        kind, fn = kinds[name]
        assert torch.isfinite(ref[name]).all(), (tag, name, "the fp64 reference is not finite")
        e, lim = fn(t, ref[name]), bar[kind] * mult
        line.append("%s %.2e" % (name, e))
        if not (torch.isfinite(t).all() and e <= lim):
            bad.append((name, e, lim))
    print("BNSTAT %s | %s" % (tag, " | ".join(line)))
    assert not bad, (tag, bad)


def _fwd_bwd(x2, dz2, bn, act, res2=None, out=None, x_view=None):
    """train_ops.bn_act forward + backward on rows x2 / dz2 [M, C] (device tensors, or `x_view`: an NCHW view to use as it is); returns what the kernels wrote"""
    x = (as_nchw(x2) if x_view is None else x_view).detach().requires_grad_(True)
    r = None if res2 is None else as_nchw(res2).detach().requires_grad_(True)
    n0 = train_ops.stats.get("native_bn_act", 0)
    y = train_ops.bn_act(x, bn, act, residual=r, out=out)
    assert train_ops.stats["native_bn_act"] == n0 + 1 and y.dtype == x.dtype
    stat = y.grad_fn.saved_tensors[3]                                              # save_mean, save_rstd: what the backward kernels will read
    y.backward(as_nchw(dz2))
    got = dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=stat[0], rstd=stat[1],
               running_mean=bn.running_mean, running_var=bn.running_var)
    if r is not None:
        got["dres"] = r.grad
    return got


def _host(got):
    return {k: (rows(v) if v.dim() == 4 else v.detach().double().cpu()) for k, v in got.items()}


def _ref(x2, dz2, bn, act, dtype, res2=None):
    """the fp64 reference of a FRESH module's first call (running statistics 0 / 1)"""
    c = x2.shape[1]
    return ref64(x2.cpu(), bn.weight.detach(), bn.bias.detach(), bn.eps, act, None if res2 is None else res2.cpu(), dz2.cpu(), bn.momentum,
                 torch.zeros(c), torch.ones(c), dtype)


# ------------------------------------------------------------------------------------------------------------------ 1. the mean / std ladder
RUNGS = [(0.4, 1.7), (4, 0.5), (8, 0.25), (-8, 0.25), (8, 1.0), (16, 0.25)]
# (pixels, channels): the size of the other BatchNorm tests (5 channel groups per slice in fp16); 4 x 160 x 160 (3 groups); 6 groups; several channel slices
SHAPES = [(4800, 72), (102400, 24), (25600, 96), (3200, 576)]


def _mult(mean, std):
    return 10 if abs(mean) / std > 32 else 1


def _seed(mean, std, M, c):
    return int(abs(mean) * 100 + std * 1000) + M + c + (7 if mean < 0 else 0)


@pytest.mark.parametrize("act", ["silu", None])
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("M,c", SHAPES)
@pytest.mark.parametrize("mean,std", RUNGS)
def test_mean_std_ladder_forward_and_backward(mean, std, M, c, dtype, act):
    """bn_act forward + backward with per-channel means of either sign around `mean` (+- 20 %) and standard deviation `std`: output, input / affine gradients, the
    saved mean / rstd and the running statistics against fp64.  |mean| / std up to 32 at the project's bars, 64 at ten times those."""
    g = torch.Generator().manual_seed(_seed(mean, std, M, c))
    x2 = ladder_rows(M, c, mean, std, dtype, _seed(mean, std, M, c))
    dz2 = torch.randn(M, c, generator=g).to(dtype)
    bn = _bn(c, g)
    ref = _ref(x2, dz2, bn, act, dtype)
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, act))
    assert int(bn.num_batches_tracked) == 1
    _check(got, ref, dtype, "ladder (%g, %g) %dx%d %s %s" % (mean, std, M, c, DTN[dtype], act), _mult(mean, std))


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("M,c", [(3200, 576), (4800, 72)])
@pytest.mark.parametrize("factor", [0.0, 4 / 9, 5.0])
def test_first_pixel_far_from_the_channel_mean(factor, M, c, dtype):
    """The (8, 0.25) rung with pixel 0 of every channel set to `factor` x the channel's mean: 0 (the value a zero-padded border can reach), 4/9 (the corner of a
    3 x 3 box filter over a constant map) and 5 (an outlier) — 32, 18 and 128 std from the mean.  bn_stats_kernel sums the squares about a pivot taken from the
    tensor; a pivot that far out brings back the cancellation of raw sums at that |mean| / std (measured with raw sums at 32: save_rstd 2.4e-4 off on the fp32
    3200 x 576 rows, bar 1e-4), so the pivot must not be pixel 0 alone.  The project's bars, as on every rung up to 32."""
    g = torch.Generator().manual_seed(M + c)
    x2 = ladder_rows(M, c, 8, 0.25, dtype, _seed(8, 0.25, M, c) + 1)
    x2[0] = (x2.double().mean(0) * factor).to(dtype)
    dz2 = torch.randn(M, c, generator=g).to(dtype)
    bn = _bn(c, g)
    ref = _ref(x2, dz2, bn, "silu", dtype)
    assert float(((x2[0].double() - ref["mean"]).abs() * ref["rstd"]).min()) > 8      # every channel's pixel 0 is many std out
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, "silu"))
    _check(got, ref, dtype, "pixel 0 = %.2f x mean %dx%d %s" % (factor, M, c, DTN[dtype]))


def _forward_ex(x, xs, M, c, dtype, bn, act, y, ys, stat, part, phase, stats_ready=0):
    lib.check(lib.load().maf_bn_forward_ex(x, xs, M, c, train_ops._DT[dtype], bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), float(bn.momentum),
                                           bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(), train_ops._ACT[act],
                                           y, ys, stat.data_ptr(), stat.data_ptr() + 4 * c, part.data_ptr(), train_ops._BN_REPLICAS, phase, None, 0, stats_ready,
                                           train_ops._stream(DEV)))


def _scratch(c):
    return torch.zeros(2 * train_ops._BN_REPLICAS * 2 * (-(-c // 256) * 256), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("mean,std", RUNGS)
def test_saved_mean_and_rstd_through_the_c_abi(mean, std, dtype):
    """maf_bn_forward_ex called directly, twice on one scratch (phase 0, then 1): save_mean / save_rstd, the running statistics after each call and y against fp64."""
    M, c = 25600, 96
    g = torch.Generator().manual_seed(11)
    bn = _bn(c, g)
    part = _scratch(c)
    rm, rv = torch.zeros(c), torch.ones(c)
    for phase in (0, 1):
        x2 = ladder_rows(M, c, mean, std, dtype, _seed(mean, std, M, c) + phase)
        xd = x2.to(DEV)
        y = torch.empty_like(xd)
        stat = torch.empty(2, c, dtype=torch.float32, device=DEV)
        _forward_ex(xd.data_ptr(), c, M, c, dtype, bn, "silu", y.data_ptr(), c, stat, part, phase)
        ref = ref64(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, "silu", None, None, bn.momentum, rm, rv, dtype)
        rm, rv = ref["running_mean"], ref["running_var"]
        got = dict(y=y.double().cpu(), mean=stat[0].double().cpu(), rstd=stat[1].double().cpu(), running_mean=bn.running_mean.double().cpu(),
                   running_var=bn.running_var.double().cpu())
        _check(got, ref, dtype, "c-abi (%g, %g) %dx%d %s phase %d" % (mean, std, M, c, DTN[dtype], phase), _mult(mean, std))
    assert int(bn.num_batches_tracked) == 2


# ------------------------------------------------------------------------------------------------------------------ 2. every producer
PRODUCER_RUNGS = [(0.4, 1.7), (8, 0.25)]


def _published(stat, bn, z, tag, dtype=F16, extra=None, ref=None):
    """the statistics an apply pass published (save_mean / save_rstd of its ctx, the module's running statistics) against the fp64 moments of the tensor `z` the
    producer actually wrote (read back from the device)"""
    z2 = rows(z)
    if ref is None:
        c = z2.shape[1]
        ref = ref64(z2, bn.weight.detach(), bn.bias.detach(), bn.eps, None, None, None, bn.momentum, torch.zeros(c), torch.ones(c), dtype)
    got = dict(mean=stat[0].double().cpu(), rstd=stat[1].double().cpu(), running_mean=bn.running_mean.double().cpu(), running_var=bn.running_var.double().cpu())
    got.update(extra or {})
    _check(got, ref, dtype, tag)
    m, v = moments(z2)
    return float((m.abs() / v.sqrt()).median())


@pytest.mark.parametrize("mean,std", PRODUCER_RUNGS)
@pytest.mark.parametrize("cin,cout,B,hw", [(64, 192, 3, (40, 40)), (48, 96, 2, (80, 80))])
def test_conv1x1_epilogue_statistics_against_fp64(cin, cout, B, hw, mean, std):
    """Conv = SiLU(BatchNorm(conv1x1(x))) with the batch statistics out of the conv's epilogue (csrc/conv_stream_lds_st.hip): what the apply pass publishes against
    the fp64 moments of the fp16 tensor the conv stored, y against fp64 BatchNorm + SiLU of that tensor.  The kernels have no bias: the pre-BatchNorm mean comes from a
    constant added to the input under positive-mean weights."""
    g = torch.Generator().manual_seed(cin + cout)
    M = B * hw[0] * hw[1]
    w = ((1 + 0.3 * torch.randn(cout, cin, 1, 1, generator=g)) / cin).to(DEV)      # z: mean ~ the input's, std ~ the input's * sqrt(1.09 / cin)
    x = (torch.randn(B, cin, *hw, generator=g) * (std * (cin / 1.09) ** 0.5) + mean).to(DEV).half().contiguous(memory_format=torch.channels_last)
    bn = _bn(cout, g)
    keys = [(M, cin, cout, cin, "st"), (M, cin, cout, cin)]
    saved = {k: train_ops._conv_tune[k] for k in keys if k in train_ops._conv_tune}
    try:
        for k in keys:
            train_ops._conv_tune[k] = (1, 4, 5)                                     # the persistent LDS-weight kernel (what the step's tuner picks for these layers)
        n0 = train_ops.stats.get("conv_bn_stats", 0)
        z, pre = train_ops.conv1x1_bn(x, w, bn)
    finally:                                                                        # the tuner's table is process-wide: later tests get the entries they would have had
        for k in keys:
            train_ops._conv_tune.pop(k, None)
        train_ops._conv_tune.update(saved)
    assert pre is not None and train_ops.stats.get("conv_bn_stats", 0) == n0 + 1
    y = train_ops.bn_act(z, bn, "silu", pre_stats=pre)
    stat = y.grad_fn.saved_tensors[3]
    z2 = rows(z)
    ref = ref64(z2, bn.weight.detach(), bn.bias.detach(), bn.eps, "silu", None, None, bn.momentum, torch.zeros(cout), torch.ones(cout), F16)
    ratio = _published(stat, bn, z, "conv1x1 epilogue %d->%d %dx%dx%d (%g, %g)" % (cin, cout, B, *hw, mean, std), extra=dict(y=rows(y)), ref=ref)
    assert ratio > 0.5 * abs(mean) / std, ratio                                     # the case is the rung it says it is


def _dw_weights(c, ks, g):
    return [((1 + 0.3 * torch.randn(c, 1, k, k, generator=g)) / (k * k)).to(DEV) for k in ks]


def _dw_weights_border_neutral(c, ks, g, a=0.3):
    """Depth-wise filters under which a zero-padded constant-plus-noise map keeps its mean at the borders: the centre tap is 1 and the other taps are noise whose
    every ROW and every COLUMN sums to zero (a double-centred Gaussian matrix, times a / k), so the taps an edge pixel lacks — whole rows or whole columns — carry
    no mean; only the (k // 2)^2 corner pixels see a remainder.  The taps still mix the neighbours (sum w^2 ~ 1 + a^2)."""
    ws = []
    for k in ks:
        r = torch.randn(c, 1, k, k, generator=g)
        r = r - r.mean(3, keepdim=True) - r.mean(2, keepdim=True) + r.mean((2, 3), keepdim=True)
        w = a * r / k
        w[:, 0, k // 2, k // 2] += 1
        ws.append(w.to(DEV))
    return ws


@pytest.mark.parametrize("mean,std", PRODUCER_RUNGS)
@pytest.mark.parametrize("k0,c,hw", [(5, 144, (20, 24)), (3, 72, (40, 40))])
def test_dw_branches_epilogue_statistics_against_fp64(k0, c, hw, mean, std):
    """The depth-wise branches of a DilatedReparamBlock in one launch whose epilogue accumulates every branch's statistics (csrc/dw_branches.hip), summed by one apply
    pass (csrc/bn_sum.hip): per branch, the published statistics against the fp64 moments of the branch tensor the kernel stored; the sum against fp64.  Zero
    padding would pull the border pixels of a constant-plus-noise map many std below the interior (a corner of a 3 x 3 box filter holds 4/9 of the mean) and
    the branch tensors' |mean| / std far below the input's on these small maps: the filters are `_dw_weights_border_neutral`, and every branch tensor is
    asserted to have the rung's ratio."""
    ks = train_ops._DWB_SETS[k0]
    g = torch.Generator().manual_seed(k0 * 100 + c)
    ws = _dw_weights_border_neutral(c, ks, g)
    sign = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
    mu = (mean * sign * (1 + 0.2 * (2 * torch.rand(c, generator=g) - 1))).view(1, c, 1, 1)
    x = (torch.randn(4, c, *hw, generator=g) * (std / 1.09 ** 0.5) + mu).to(DEV).half().contiguous(memory_format=torch.channels_last)
    bns = [_bn(c, g) for _ in ks]
    n0 = train_ops.stats.get("native_bn_sum", 0)
    zz, pre = train_ops.dw_branches(x, ws, bns)
    assert all(p is not None for p in pre)
    y = train_ops.bn_sum(zz, bns, pre)
    assert train_ops.stats.get("native_bn_sum", 0) == n0 + 1
    stat = y.grad_fn.saved_tensors[0]                                              # [branch][save_mean, save_rstd][c]
    total = 0
    for j, (z, bn) in enumerate(zip(zz, bns)):
        ratio = _published(stat[j], bn, z, "dw_branches k0=%d c=%d %dx%d (%g, %g) branch %d" % (k0, c, *hw, mean, std, j))
        assert ratio > 0.5 * abs(mean) / std, (j, ratio)                            # the case is the rung it says it is
        total = total + ref64(rows(z), bn.weight.detach(), bn.bias.detach(), bn.eps)["y"]
    e = err_max(rows(y), total.half().double())
    print("BNSTAT dw_branches sum k0=%d c=%d (%g, %g) | y %.2e" % (k0, c, mean, std, e))
    assert e <= bn_ref.BARS[F16]["y"], e


@pytest.mark.parametrize("mean,std", PRODUCER_RUNGS)
def test_branch_sum_stats_form_statistics_against_fp64(mean, std):
    """UniRepLKNetBlock = norm(DilatedReparamBlock(x)): the apply pass that writes the branch sum (maf_bn_sum_forward_stats) accumulates norm's batch statistics.
    What norm's apply pass publishes against the fp64 moments of the stored sum; the pre-norm mean / std are set through the branches' beta / gamma."""
    from maf_yolo_amd.layers import UniRepLKNetBlock
    c, k, hw = 96, 9, (20, 20)
    g = torch.Generator().manual_seed(c + k)
    blk = UniRepLKNetBlock(c, k).to(DEV).train()
    names = ["lk_origin"] + ["dil_conv_k%d_1" % kk for kk in blk.dwconv.kernel_sizes]
    bns = [blk.dwconv.origin_bn] + [getattr(blk.dwconv, "dil_bn_k%d_1" % kk) for kk in blk.dwconv.kernel_sizes]
    nb = len(bns)
    with torch.no_grad():
        for n_, w in zip(names, _dw_weights(c, [k] + list(blk.dwconv.kernel_sizes), g)):
            getattr(blk.dwconv, n_).weight.copy_(w)
        sign = (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1).to(DEV)
        for bn in bns:                                                              # sum of nb unit-variance branches: std ~ gamma sqrt(nb), mean = nb beta
            bn.weight.fill_(std / nb ** 0.5)
            bn.bias.copy_(sign * mean / nb * (1 + 0.2 * (2 * torch.rand(c, generator=g) - 1)).to(DEV))
        blk.norm.weight.copy_((torch.rand(c, generator=g) + 0.5).to(DEV))
        blk.norm.bias.copy_((torch.randn(c, generator=g) * 0.3).to(DEV))
    x = (torch.randn(4, c, *hw, generator=g) * 1.5 + 0.2).to(DEV).half().contiguous(memory_format=torch.channels_last)
    n0 = train_ops.stats.get("bn_sum_next_stats", 0)
    s, pre = blk.dwconv(x, next_bn=blk.norm)
    assert pre is not None and train_ops.stats.get("bn_sum_next_stats", 0) == n0 + 1
    y = train_ops.bn_act(s, blk.norm, "silu", pre_stats=pre)
    stat = y.grad_fn.saved_tensors[3]
    ref = ref64(rows(s), blk.norm.weight.detach(), blk.norm.bias.detach(), EPS, "silu", None, None, MOM, torch.zeros(c), torch.ones(c), F16)
    ratio = _published(stat, blk.norm, s, "bn_sum STATS c=%d k=%d %dx%d (%g, %g)" % (c, k, *hw, mean, std), extra=dict(y=rows(y)), ref=ref)
    assert ratio > 0.5 * abs(mean) / std, ratio


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("mean,std", PRODUCER_RUNGS)
def test_bn_stats_entry_point_on_a_channel_slice(mean, std, dtype):
    """maf_bn_stats (the statistics launch of a branch without an epilogue) on a channel slice of a wider NHWC buffer whose other channels are NaN, then the
    apply pass alone (stats_ready): the published statistics and y against fp64 of the slice."""
    M, c, lo, wide = 4800, 72, 16, 104
    g = torch.Generator().manual_seed(21)
    x2 = ladder_rows(M, c, mean, std, dtype, _seed(mean, std, M, c))
    buf = torch.full((M, wide), float("nan"), dtype=dtype, device=DEV)
    buf[:, lo:lo + c] = x2.to(DEV)
    bn = _bn(c, g)
    part = _scratch(c)
    es = buf.element_size()
    lib.check(lib.load().maf_bn_stats(buf.data_ptr() + lo * es, wide, M, c, train_ops._DT[dtype], part.data_ptr(), train_ops._BN_REPLICAS, 0, train_ops._stream(DEV)))
    y = torch.empty(M, c, dtype=dtype, device=DEV)
    stat = torch.empty(2, c, dtype=torch.float32, device=DEV)
    _forward_ex(buf.data_ptr() + lo * es, wide, M, c, dtype, bn, None, y.data_ptr(), c, stat, part, 0, stats_ready=1)
    ref = ref64(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, None, None, None, bn.momentum, torch.zeros(c), torch.ones(c), dtype)
    got = dict(y=y.double().cpu(), mean=stat[0].double().cpu(), rstd=stat[1].double().cpu(), running_mean=bn.running_mean.double().cpu(),
               running_var=bn.running_var.double().cpu())
    _check(got, ref, dtype, "maf_bn_stats slice (%g, %g) %s" % (mean, std, DTN[dtype]))


# ------------------------------------------------------------------------------------------------------------------ 3. the scratch protocol
_ACTS = ["silu", None]          # (no ReLU over these 3.7 M-element calls: an element whose u is within fp32 round-off of 0 has no decisive reference for its mask)


def _sequence(seed):
    """24 calls cycling the widths 24, 200 (5 replicas), 256, 264, 768 (1 replica), 1032 (1024 / C = 0), 24 (16 replicas) with M in {37, 1, 4800} and fp16 / fp32 rows
    in alternation — 24, 200 and 256 share one scratch buffer whatever the dtype —, every C = 200 call with an input 1e4 times larger, plus one more such call in
    front of a C = 24 call that has one behind it already.  Host tensors; the reference of each call."""
    calls = []
    widths, Ms = [24, 200, 256, 264, 768, 1032, 24], [37, 1, 4800]
    for i in range(24):
        calls.append(dict(c=widths[i % 7], M=Ms[i % 3], dtype=F16 if i % 2 == 0 else F32, act=_ACTS[(i // 2) % 2]))
    assert calls[7]["c"] == 24 and calls[7]["M"] == 1 and calls[8]["c"] == 200
    calls.insert(7, dict(c=200, M=4800, dtype=F16, act="silu"))
    g = torch.Generator().manual_seed(seed)
    for i, k in enumerate(calls):
        c, M, dtype = k["c"], k["M"], k["dtype"]
        if c == 200:
            k["x2"] = ((torch.randn(M, c, generator=g) * 0.3 + 1.0) * 1e4).to(dtype)       # (below fp16's largest finite value)
        else:
            k["x2"] = ladder_rows(M, c, 0.4, 1.7, dtype, seed * 100 + i)
        k["dz2"] = torch.randn(M, c, generator=g).to(dtype)
        k["gamma"], k["beta"] = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
        k["ref"] = ref64(k["x2"], k["gamma"], k["beta"], EPS, k["act"], None, k["dz2"], MOM, torch.zeros(c), torch.ones(c), dtype)
    return calls


def _module(k):
    bn = torch.nn.BatchNorm2d(k["c"], eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.weight.copy_(k["gamma"]); bn.bias.copy_(k["beta"])
    return bn.to(DEV).train()


def _check_sequence(calls, gots, tag):
    for i, (k, got) in enumerate(zip(calls, gots)):
        got = dict(got)
        got.pop("mean"), got.pop("rstd")                                            # (the saved statistics: sections 1 and 2)
        _check(_host(got), {n: k["ref"][n] for n in got}, k["dtype"], "%s call %d C=%d M=%d %s %s" % (tag, i, k["c"], k["M"], DTN[k["dtype"]], k["act"]))


@pytest.mark.parametrize("deterministic", [False, True])
def test_scratch_protocol_over_a_sequence_of_widths(deterministic):
    """25 bn_act forward + backward calls of different widths, pixel counts and dtypes on one stream (`_sequence`), no tape, each against fp64 — with the fp32 atomics
    and in deterministic mode (per-workgroup slots; replica 0 is stored, the other replicas must have stayed zero).

    Why a skipped `part_clear` store fails this test: a call accumulates into half `phase` of the buffer its width shares and its apply pass zeroes ALL of the other
    half (clear_n = the half), the half the next call accumulates into.  The C = 200 calls use replicas 0..4 of [R][2][200], floats 0..1999 of a half; their inputs are
    ~1e4, so each of those floats holds about 1e4 * M / 5 (sum x) or 1e8 * M / 5 (sum x^2), M = 4800 for the call in front of the C = 24, M = 1 one.  The C = 24
    call reads replicas 0..15 of [R][2][24], floats 0..767 of the same halves: ANY float there left uncleared by the forward (or backward) pass between them adds
    >= 1e4 * 4800 / 5 ~ 1e7 to a sum of one value of size ~1 — mean and variance of that channel are off by seven orders of magnitude against a bar of 1e-4, and the
    backward sums {sum g, sum g xhat} likewise.  The second C = 200 call behind it, and the wider calls that use 1 replica after calls that used 16, catch the same in
    the other direction (floats 768..1999 / the replicas beyond the first)."""
    calls = _sequence(3)
    mods = [_module(k) for k in calls]
    dev = [(k["x2"].to(DEV), k["dz2"].to(DEV)) for k in calls]
    if deterministic:
        train_ops.set_deterministic(True)
    try:
        gots = [_fwd_bwd(x2, dz2, bn, k["act"]) for k, bn, (x2, dz2) in zip(calls, mods, dev)]
        torch.cuda.synchronize()
    finally:
        if deterministic:
            train_ops.set_deterministic(False)
    _check_sequence(calls, gots, "sequence det" if deterministic else "sequence")


def test_scratch_phases_on_the_step_tape():
    """The same sequence recorded on a step tape (maf_yolo_amd/tape.py) and replayed twice with new inputs: under a recording every call site owns its scratch and its
    phase is a word that tape.toggle flips between replays (train_ops._bn_part, lib.Phase) instead of a Python counter.  The recorded run and both replays against
    fp64: a phase that did not alternate accumulates onto the sums its own last run left behind (errors of order one)."""
    runs = [_sequence(5 + r) for r in range(3)]
    calls = runs[0]
    mods = [_module(k) for k in calls]
    xs = [as_nchw(k["x2"].to(DEV)).detach().requires_grad_(True) for k in calls]
    dzs = [as_nchw(k["dz2"].to(DEV)) for k in calls]
    tp = tape_mod.StepTape(None, DEV)
    try:
        tp.begin("fwd")
        try:
            ys = [train_ops.bn_act(x, bn, k["act"]) for k, bn, x in zip(calls, mods, xs)]
        finally:
            tp.end()
        tp._finalise("fwd")
        stats = [y.grad_fn.saved_tensors[3] for y in ys]
        tp.begin("bwd")
        try:
            grads = [torch.autograd.grad(y, (x, bn.weight, bn.bias), dz) for y, x, bn, dz in zip(ys, xs, mods, dzs)]
        finally:
            tp.end()
        tp._finalise("bwd")
        assert tp.n["fwd"] == len(calls) and tp.n["bwd"] == len(calls), tp.n
        assert len(tp.tog["fwd"][0]) >= len(calls) and tp.tog["fwd"][1] == len(calls) and tp.tog["bwd"][1] == len(calls)

        def results():
            torch.cuda.synchronize()
            return [dict(y=y.detach(), dx=gr[0], dgamma=gr[1], dbeta=gr[2], mean=st[0], rstd=st[1], running_mean=bn.running_mean, running_var=bn.running_var)
                    for y, gr, st, bn in zip(ys, grads, stats, mods)]
        _check_sequence(calls, results(), "tape record")
        for r in (1, 2):
            with torch.no_grad():
                for k, x, dz, bn in zip(runs[r], xs, dzs, mods):
                    x.copy_(as_nchw(k["x2"].to(DEV))); dz.copy_(as_nchw(k["dz2"].to(DEV)))
                    bn.weight.copy_(k["gamma"]); bn.bias.copy_(k["beta"])
                    bn.running_mean.zero_(); bn.running_var.fill_(1)
            tp._run("fwd", 0, tp.n["fwd"])
            tp._toggle("fwd")
            tp._run("bwd", 0, tp.n["bwd"])
            tp._toggle("bwd")
            _check_sequence(runs[r], results(), "tape replay %d" % r)
        assert all(int(bn.num_batches_tracked) == 3 for bn in mods)
    finally:
        tp.release()


# ------------------------------------------------------------------------------------------------------------------ 4. geometry and value edges
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("act", ["silu", None])
def test_one_pixel_per_channel(dtype, act):
    """M = 1: the batch variance is 0, y = act(beta), dx = 0, and running_var takes the BIASED value (bn_apply_kernel's guard for M = 1; torch raises for one value
    per channel, so the rule as documented is the reference)."""
    c = 72
    g = torch.Generator().manual_seed(1)
    x2, dz2 = ladder_rows(1, c, 0.4, 1.7, dtype, 1), torch.randn(1, c, generator=g).to(dtype)
    bn = _bn(c, g)
    ref = _ref(x2, dz2, bn, act, dtype)
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert float(ref["var"].abs().max()) == 0 and torch.equal(ref["running_var"], torch.full((c,), 1 - MOM, dtype=torch.float64))
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, act))
    _check(got, ref, dtype, "M=1 %s %s" % (DTN[dtype], act))


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("M,c", [(3, 2048), (513, 72), (37, 24), (4127, 200)])
def test_pixel_counts_off_the_lane_and_unroll_grid(M, c, dtype):
    """Fewer pixels than pixel lanes with the widest layer (3 x 2048), one more than a multiple of the lane count x unroll (513), an odd count over a
    non-power-of-two group count (37 x 24; 4127 x 200: several workgroups, ragged last chunk)."""
    g = torch.Generator().manual_seed(M + c)
    x2, dz2 = ladder_rows(M, c, 0.4, 1.7, dtype, M + c), torch.randn(M, c, generator=g).to(dtype)
    bn = _bn(c, g)
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, "silu"))
    _check(got, _ref(x2, dz2, bn, "silu", dtype), dtype, "geometry %dx%d %s" % (M, c, DTN[dtype]))


@pytest.mark.parametrize("dtype", [F32, F16])
def test_constant_and_zero_channels(dtype):
    """A channel constant at 5.0 (variance exactly 0: y = act(beta) up to rounding, dx finite) and a channel of exact zeros among ordinary ones."""
    M, c = 4800, 72
    g = torch.Generator().manual_seed(8)
    x2, dz2 = ladder_rows(M, c, 0.4, 1.7, dtype, 8), torch.randn(M, c, generator=g).to(dtype)
    x2[:, 5] = 5.0
    x2[:, 17] = 0.0
    bn = _bn(c, g)
    ref = _ref(x2, dz2, bn, "silu", dtype)
    assert all(torch.isfinite(v).all() for v in ref.values()) and float(ref["var"][5]) == 0 and float(ref["var"][17]) == 0
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, "silu"))
    assert torch.isfinite(got["dx"]).all()
    _check(got, ref, dtype, "constant / zero channel %s" % DTN[dtype])
    beta = bn.bias.detach().double().cpu()
    want = bn_ref.store(beta * torch.sigmoid(beta), dtype)
    for ch in (5, 17):                                                             # the channel on its own: SiLU(beta), at the bar in units of the tensor's largest output
        e = float((got["y"][:, ch] - want[ch]).abs().max()) / float(ref["y"].abs().max())
        assert e <= bn_ref.BARS[dtype]["y"], (ch, e)


@pytest.mark.parametrize("dtype", [F32, F16])
def test_silu_backward_over_a_wide_pre_activation_range(dtype):
    """gamma = 12: the pre-activation u spans more than [-30, 30], where exp(-u) leaves fp32's comfortable range on one side and the gradient is 1 on the other."""
    M, c = 4800, 24
    g = torch.Generator().manual_seed(12)
    x2, dz2 = ladder_rows(M, c, 0.4, 1.7, dtype, 12), torch.randn(M, c, generator=g).to(dtype)
    bn = _bn(c, g, gamma=12)
    ref = _ref(x2, dz2, bn, "silu", dtype)
    xh = (x2.double() - ref["mean"]) * ref["rstd"]
    assert float((xh * 12).min()) < -30 and float((xh * 12).max()) > 30
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, "silu"))
    _check(got, ref, dtype, "silu range %s" % DTN[dtype])


@pytest.mark.parametrize("dtype,act", [(F32, "relu"), (F16, None), (F16, "relu")])
def test_residual_against_fp64(dtype, act):
    """act(BatchNorm(x) + residual): output and the gradients of x, the residual, gamma and beta against fp64."""
    M, c = 513, 72
    g = torch.Generator().manual_seed(30)
    x2, dz2 = ladder_rows(M, c, 4, 0.5, dtype, 30), torch.randn(M, c, generator=g).to(dtype)
    r2 = torch.randn(M, c, generator=g).to(dtype)
    bn = _bn(c, g)
    if act == "relu":                                                              # a decisive reference: no pre-activation within 1e-3 of the ReLU's kink (the kernel's fp32 u is ~1e-6 off)
        for _ in range(8):
            o = ref64(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, None, r2, None, None, None, None)
            near = o["y"].abs() < 1e-3
            if not near.any():
                break
            r2 = torch.where(near, r2 + 2.0 ** -6, r2).to(dtype)
        assert not near.any()
    got = _host(_fwd_bwd(x2.to(DEV), dz2.to(DEV), bn, act, res2=r2.to(DEV)))
    ref = _ref(x2, dz2, bn, act, dtype, res2=r2)
    if act is None:
        ref["dres"] = dz2.double()                                                 # no activation: the upstream gradient itself
    _check(got, ref, dtype, "residual %s %s" % (DTN[dtype], act))


@pytest.mark.parametrize("dtype", [F32, F16])
def test_channel_slice_input_into_a_concat_slot(dtype):
    """The input a channel slice of a wider NHWC buffer (pixel stride != C), out= a slot of a concat buffer (CatBuffer.slot): the other channels of both buffers are
    NaN before and bit-identical afterwards; the slot and the gradients against fp64."""
    M, c, lo, wide = 513, 72, 8, 96
    g = torch.Generator().manual_seed(40)
    x2, dz2 = ladder_rows(M, c, 0.4, 1.7, dtype, 40), torch.randn(M, c, generator=g).to(dtype)
    src = torch.full((M, wide), float("nan"), dtype=dtype)
    src[:, lo:lo + c] = x2
    src = src.to(DEV)
    src0 = src.clone()
    cb = train_ops.CatBuffer(train_ops.Like((1, 0, 1, M), dtype, DEV), [16, c, 24])
    cb.buf.fill_(float("nan"))
    buf0 = cb.buf.clone()
    bn = _bn(c, g)
    xv = as_nchw(src)[:, lo:lo + c]
    assert train_ops.nhwc(xv)[1] == wide
    glue0 = train_ops.stats.get("glue", 0)
    got = _fwd_bwd(None, dz2.to(DEV), bn, "silu", out=cb.slot(1), x_view=xv)
    torch.cuda.synchronize()
    assert train_ops.stats.get("glue", 0) == glue0                                  # no copy to a dense tensor on the way
    it = torch.int16 if dtype == F16 else torch.int32
    assert torch.equal(src.view(it), src0.view(it))
    bits, bits0 = rows(cb.buf.view(it)).long(), rows(buf0.view(it)).long()
    assert torch.equal(bits[:, :16], bits0[:, :16]) and torch.equal(bits[:, 16 + c:], bits0[:, 16 + c:])
    assert got["y"].data_ptr() == cb.buf.data_ptr() + 16 * cb.buf.element_size()
    got["y"] = cb.buf[:, 16:16 + c]
    _check(_host(got), _ref(x2, dz2, bn, "silu", dtype), dtype, "slice -> slot %s" % DTN[dtype])
