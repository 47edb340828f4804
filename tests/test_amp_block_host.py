"""Host-side checks (no GPU) of tests/amp_block_ref.py, the yardstick of tests/test_gpu_amp_blocks.py:

  * the unit enumeration covers every trainable parameter of n, s and m exactly once;
  * the fp64 reference of one unit of every kind agrees to 1e-5 with the package's own CPU path (plain torch in layers.py) in fp32 — y, dx, every parameter gradient;
  * the coverage holds for the reference alone: one CPU fp32 train step of n leaves no parameter gradient all-zero (synth_state_dict gives non-zero prediction weights);
  * Bar B has teeth: on a Conv unit and a UniRepLKNetBlock unit at m's widths, with "framework" = the fp64 reference rounded to fp16 once, two planted defects — batch statistics
    over all pixels but the last one, a weight gradient that misses the last pixel row — are over the bar, and the once-rounded reference under another summation order is inside it."""
import pytest
import torch

import maf_yolo_amd as M
from maf_yolo_amd import train_ops
from oracle import maf_oracle as O

import amp_block_ref as R

_TARGETS = [[0, 3, 0.40, 0.50, 0.30, 0.40], [0, 17, 0.70, 0.30, 0.20, 0.50], [0, 17, 0.25, 0.75, 0.30, 0.25],
            [1, 5, 0.50, 0.50, 0.60, 0.60], [1, 62, 0.20, 0.30, 0.25, 0.35]]          # tests/test_gpu_train.py::_TRAIN_TARGETS


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(scale):
        if scale not in cache:
            m = M.Model(scale)
            m.load_state_dict(O.synth_state_dict(scale, 0))
            cache[scale] = m.train()
        return cache[scale]
    return get


@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_every_trainable_parameter_belongs_to_exactly_one_unit(models, scale):
    m = models(scale)
    us = R.units(m)
    assert {u.kind for u in us} == set(R.KINDS)
    assert len({u.name for u in us}) == len(us)
    owner = {}
    for u in us:
        for n, p in u.params:
            assert id(p) not in owner, (u.name, n, owner[id(p)])
            owner[id(p)] = u.name + "." + n
    missing = [k for k, p in m.named_parameters() if p.requires_grad and id(p) not in owner]
    assert not missing, missing
    assert len(owner) == sum(1 for p in m.parameters() if p.requires_grad)
    # every BatchNorm of the model is some unit's, once
    bns = [id(b) for u in us for _, b in u.bns]
    assert len(bns) == len(set(bns)) == sum(1 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    # the stages partition the units; the count of compared pairs follows from the enumeration alone
    assert sum(len([u for u in us if R.in_stage(u, st)]) for st in R.STAGES) == len(us)
    assert R.predicted_pairs(us) == sum(len(u.keys(False)) + len(u.keys(True)) for u in us)
    # the units the cat-free path reaches without a module call
    direct = [u for u in us if u.direct]
    assert sum(1 for u in direct if u.kind == "pred") == 6
    assert sum(1 for u in direct if u.kind == "conv1x1") == sum(1 for mod in m.modules() if type(mod).__name__ == "RepHDW")


def _first(us, kind, pick=None):
    return next(u for u in us if u.kind == kind and (pick is None or pick(u)))


def _one_of_each_kind(us):
    return [_first(us, "conv1x1", lambda u: not u.direct), _first(us, "conv1x1", lambda u: u.direct), _first(us, "conv3x3s2"), _first(us, "repvgg", lambda u: u.node > 0),
            _first(us, "repvgg", lambda u: u.node == 0), _first(us, "unirep", lambda u: u.act == "silu"), _first(us, "unirep", lambda u: u.act is None),
            _first(us, "sppf_pool"), _first(us, "mp"), _first(us, "pred")]


def _cin(u):
    if u.kind in ("conv1x1", "conv3x3s2"):
        return u.module.conv.in_channels
    if u.kind == "repvgg":
        return u.module.rbr_dense.conv.in_channels
    if u.kind == "unirep":
        return u.module.norm.num_features
    if u.kind == "sppf_pool":
        return u.module.cv1.conv.out_channels
    if u.kind == "pred":
        return u.module.in_channels
    return 16


def test_reference_agrees_with_the_cpu_path_of_the_package_in_fp32(models):
    """On CPU tensors layers.py is plain torch: the same unit, fp32, against the fp64 restatement — 1e-5 of max |ref| on y, dx, every parameter gradient and the running statistics."""
    m = models("n")
    g = torch.Generator().manual_seed(11)
    seen = set()
    for u in _one_of_each_kind(R.units(m)):
        seen.add(u.kind)
        x = torch.randn(2, _cin(u), 12, 10, generator=g) * (2.0 if u.kind != "repvgg" else 0.5)
        pre = {n: (b.running_mean.clone(), b.running_var.clone()) for n, b in u.bns}
        for _, p in u.params:
            p.grad = None
        xr = x.clone().requires_grad_()
        y = R.run_unit(u, xr, train_ops)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        got = {"y": y, "dx": xr.grad}
        for n, p in u.params:
            got["g:" + n] = p.grad
        for n, b in u.bns:
            got["rm:" + n], got["rv:" + n] = b.running_mean, b.running_var
        # (fp32 in: the reference must not round this input to fp16 — hand it over as fp64)
        ref = R.reference(u, x.double(), dy, pre)
        e = R.errors(got, ref, u.keys(True))
        assert max(e.values()) <= 1e-5, (u, e)
        for n, b in u.bns:                                    # leave the shared model as it was
            b.running_mean.copy_(pre[n][0]); b.running_var.copy_(pre[n][1])
        for _, p in u.params:
            p.grad = None
    assert seen == set(R.KINDS)


@pytest.mark.parametrize("size", [128, 192])
def test_cpu_fp32_step_reaches_every_parameter_the_loss_depends_on(models, size):
    """One fp32 train step of n on the CPU (plain torch modules, the oracle's loss with the warm-up assigner, which the GPU audit's ComputeLoss runs at epoch 0): every parameter
    gradient is finite, and the ONLY all-zero ones are where the loss does not depend on the parameter — the box branch (reg_conv, reg_conv_s, reg_pred) of a head on whose level the
    assigner put no foreground anchor: the box losses are sums over the foreground anchors alone.  With the five labels of the end-to-end test that is the stride-32 head at 128 x 128
    (a 4 x 4 map) and no head at 192 x 192; the task-aligned assigner would leave the stride-16 head without one too, which is why the audit runs the warm-up one.  The GPU audit
    asserts the same rule on the device's own assignment and replays those units with a stand-in gradient (tests/test_gpu_amp_blocks.py)."""
    m = models("n")
    m.zero_grad(set_to_none=True)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    (feats, cls, reg), _ = m(O.synth_images(2, size, 7))
    hw = [tuple(f.shape[-2:]) for f in feats]
    loss, _, (_, _, _, fg) = O.compute_loss(hw, cls, reg, torch.tensor(_TARGETS), img_size=size, assigner="atss", return_assignment=True)
    loss.backward()
    try:
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
        dead = {k for k, p in m.named_parameters() if p.requires_grad and float(p.grad.abs().max()) == 0.0}
        heads = [u.name.rsplit(".", 1)[0] for u in R.units(m) if u.name.endswith(".cls_pred")]
        a0, allowed = 0, set()
        for head, (h, w) in zip(heads, hw):
            if int(fg[:, a0:a0 + h * w].sum()) == 0:
                allowed |= {k for k, _ in m.named_parameters() if k.startswith(head + ".reg_")}
            a0 += h * w
        assert dead == allowed, sorted(dead ^ allowed)
        assert allowed == ({k for k, _ in m.named_parameters() if k.startswith("backbone.33.reg_")} if size == 128 else set())
    finally:
        m.load_state_dict(sd0)
        m.zero_grad(set_to_none=True)


def _h(t):
    return t.to(torch.float16).double()


def _planted(u, shape, seed):
    """(ref, fw, reordered, stats defect, wgrad defect): {key: tensor} of unit u on a random fp16 input of `shape` — the fp64 reference; the same rounded to fp16 once (y, dx; the
    parameter gradients too: the framework's convolution hands its weight gradient over in fp16); the reference summed in another order (mirrored maps: every tap and pixel sum runs
    backwards), rounded once; y with every BatchNorm's statistics taken over all pixels but the last one; the conv weight gradients from a dy without its last pixel row."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * 1.5).to(torch.float16)
    P = {n: p.detach().double() for n, p in u.params}
    y0 = R.forward64(u, x.double(), P)
    dy = (torch.randn(y0.shape, generator=g) * 0.05).to(torch.float16)
    ref = R.reference(u, x, dy)
    keys = u.keys(True)[: 2 + len(u.params)]                 # y, dx, parameter gradients (no running statistics without a `pre`)
    fw = {k: _h(ref[k]) for k in keys}
    # another summation order: the unit on the mirrored input with mirrored filters and gradient, mirrored back
    flip = lambda t: t.flip(-1, -2) if t.dim() == 4 else t
    x64 = flip(x.double()).requires_grad_()
    Pf = {n: flip(p).clone().requires_grad_() for n, p in P.items()}
    yf = R.forward64(u, x64, Pf)
    yf.backward(flip(dy.double()))
    reo = {"y": _h(flip(yf.detach())), "dx": _h(flip(x64.grad))}
    for n in P:
        reo["g:" + n] = _h(flip(Pf[n].grad))
    # defect 1: statistics over all pixels but the last one
    stats = {}
    R.forward64(u, x.double(), P, stats)
    mom = {}
    for n, _ in u.bns:
        z = _bn_input(u, x.double(), P, n)
        rows = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])[:-1]
        mean = rows.mean(0)
        mom[n] = (mean, ((rows - mean) ** 2).mean(0))
    d_stats = dict(fw)
    d_stats["y"] = _h(R.forward64(u, x.double(), P, moments=mom))
    # defect 2: a weight gradient that misses the last pixel row
    dy_cut = dy.clone()
    dy_cut[:, :, -1, :] = 0
    cut = R.reference(u, x, dy_cut)
    d_wgrad = dict(fw)
    for n, p in u.params:
        if p.dim() == 4:
            d_wgrad["g:" + n] = _h(cut["g:" + n])
    return ref, fw, reo, d_stats, d_wgrad, keys


def _bn_input(u, x, P, tag):
    """the tensor BatchNorm `tag` of the unit normalises (fp64): the unit's forward up to it"""
    import torch.nn.functional as F
    m = u.module
    if u.kind == "conv1x1":
        return F.conv2d(x, P["conv.weight"])
    c, d = x.shape[1], m.dwconv
    convs = {"dwconv.origin_bn": ("dwconv.lk_origin.weight", d.kernel_size)}
    for kk in d.kernel_sizes:
        convs["dwconv.dil_bn_k%d_1" % kk] = ("dwconv.dil_conv_k%d_1.weight" % kk, kk)
    if tag in convs:
        w, k = convs[tag]
        return F.conv2d(x, P[w], None, 1, k // 2, 1, c)
    s = 0
    for t, (w, k) in convs.items():
        s = s + R.bn_batch(F.conv2d(x, P[w], None, 1, k // 2, 1, c), P[t + ".weight"], P[t + ".bias"], dict(u.bns)[t].eps)[0]
    return s


@pytest.mark.parametrize("kind", ["conv1x1", "unirep"])
def test_bar_b_trips_on_planted_defects_and_passes_a_reordered_sum(models, kind):
    """m's widths on its stride-32 map (2 x C x 4 x 4: 32 values per channel, where one dropped pixel moves a mean the most)."""
    us = R.units(models("m"))
    u = _first(us, kind, lambda u_: 5 <= u_.node <= 9 and not u_.direct)      # backbone.8 / backbone.9: the widest maps of the backbone
    ref, fw, reo, d_stats, d_wgrad, keys = _planted(u, (2, _cin(u), 4, 4), 5)
    e_fw = R.errors(fw, ref, keys)
    assert max(e_fw.values()) <= 2.0 ** -11 * 1.001, e_fw       # rounded once: half an ulp of the largest value
    # the reordered sum is inside both bars
    assert not R.judge(R.errors(reo, ref, keys), e_fw)
    # statistics without the last pixel: y is over Bar B
    bad = R.judge(R.errors(d_stats, ref, keys), e_fw)
    assert [b for b in bad if b[0] == "y"], (bad, R.errors(d_stats, ref, keys))
    # weight gradient without the last pixel row: every conv weight's gradient is over a bar
    bad = {b[0] for b in R.judge(R.errors(d_wgrad, ref, keys), e_fw)}
    convw = {"g:" + n for n, p in u.params if p.dim() == 4}
    assert convw and convw <= bad, (convw, bad)


def test_bars_are_the_projects_fp16_bars():
    assert (R.bar_a("y"), R.bar_a("dx"), R.bar_a("g:conv.weight"), R.bar_a("rv:bn")) == (1e-2, 2e-2, 2e-2, 2e-3)
    assert R.bar_b(0.0) == 2.0 ** -10 and R.bar_b(1e-3) == 1.5e-3 + 2.0 ** -10
    # a design difference's own bar replaces Bar B only
    assert R.judge({"y": 3e-3}, {"y": 1e-4}) == [("y", 3e-3, 1e-4, "B")]
    assert R.judge({"y": 3e-3}, {"y": 1e-4}, own={"y": 4e-3}) == []
    assert R.judge({"y": 2e-2}, {"y": 1e-4}, own={"y": 1.0}) == [("y", 2e-2, 1e-4, "A")]
