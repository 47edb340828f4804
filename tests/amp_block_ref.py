"""Block-local audit of one AMP (fp16 autocast) train step: the units of the train-form graph, their plain fp64 references, and the error / bar helpers of
tests/test_gpu_amp_blocks.py (GPU) and tests/test_amp_block_host.py (CPU).

A UNIT is one conv / BatchNorm / activation group as maf-yolo_amd/layers.py composes it:

    conv1x1, conv3x3s2   every `Conv`: conv -> BatchNorm (batch statistics) -> SiLU
    repvgg               every `RepVGGBlock`: ReLU(BN(conv3x3 s2) + BN(conv1x1 s2))
    unirep               every `UniRepLKNetBlock`: sum_j BN_j(depth-wise conv_j) -> BN (norm) -> the activation handed in (SiLU inside DepthBottleneckUni, none in the heads)
    sppf_pool            SPPF's three chained 5 x 5 max-pools between cv1 and cv2: y = cat(p1, p2, p3)
    mp                   the 2 x 2 stride-2 max-pool of MPRep
    pred                 cls_pred / reg_pred of every head: 1x1 conv with a bias

Every parameter with requires_grad belongs to exactly one unit (test_amp_block_host.py asserts it for n, s and m).

The reference of a unit is evaluated ON THE UNIT'S OWN STORED INPUT (the fp16 values the kernel read, converted exactly to fp64) and its backward is fp64 autograd on the stored
upstream gradient: nothing upstream or downstream of the unit is in the comparison, so nothing amplifies — a correct fp16 block sits within a few fp16 ulps of it.  Weights are the fp32
master parameters (the fp16 cast of the weights is part of the error of whoever runs the block in fp16).  BatchNorm is written out with the two-pass mean / biased variance of
tests/bn_ref.py.  Nothing here touches the package's training ops: `run_unit` takes them as an argument from the caller.

Tensor keys of a unit:  y, dx, g:<parameter> (its gradient), rm:<bn> / rv:<bn> (running_mean / running_var after the step: what the unit exposes of its batch statistics).
Error: bn_ref.err_max = max |got - ref64| / max |ref64|.
Bar A (gross, absolute): the project's fp16 bars, bn_ref.BARS[torch.float16] — y 1e-2, gradients 2e-2, statistics 2e-3.
Bar B (local, relative):  e_hip <= 1.5 * e_fw + 2**-10, e_fw the error of the SAME unit on the SAME stored tensors run on the framework's ops under the same autocast; 1.5 is the factor the
end-to-end test applies to n and s, 2**-10 one fp16 ulp at the tensor's largest value (two correctly rounded results may differ by that)."""
import torch
import torch.nn.functional as F

import bn_ref

BAR_A = bn_ref.BARS[torch.float16]
BAR_B_MULT, BAR_B_ULP = 1.5, 2.0 ** -10
STAGES = {"backbone": (0, 8), "neck": (9, 30), "heads": (31, 10 ** 9)}           # the node ranges of tests/test_gpu_train.py::_train_step_vs_reference
KINDS = ("conv1x1", "conv3x3s2", "repvgg", "unirep", "sppf_pool", "mp", "pred")


class Unit:
    """name: the module path; module: what holds the unit's hyper-parameters; params / bns: [(name inside the module, tensor / BatchNorm2d)]; act: the activation behind the last
    BatchNorm; direct: the cat-free path does not go through the module's __call__ (RepHDW.conv1: train_ops.conv1x1 + train_ops.bn_act; the prediction convs: train_ops.conv1x1)."""

    def __init__(self, name, kind, module, act=None, direct=False):
        self.name, self.kind, self.module, self.act, self.direct = name, kind, module, act, direct
        if kind in ("sppf_pool", "mp"):
            self.params, self.bns = [], []
        else:
            self.params = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
            self.bns = [(n, b) for n, b in module.named_modules() if isinstance(b, torch.nn.BatchNorm2d)]
        self.node = int(name.split(".")[1])

    def keys(self, replay):
        """the tensors compared for this unit: in place (replay False) y, the parameter gradients and the running statistics; the replay adds dx"""
        ks = ["y"] + (["dx"] if replay else []) + ["g:" + n for n, _ in self.params]
        for n, _ in self.bns:
            ks += ["rm:" + n, "rv:" + n]
        return ks

    def __repr__(self):
        return "Unit(%s, %s)" % (self.name, self.kind)


def units(model):
    """every audited unit of a maf_yolo_amd.Model, in module order"""
    out = []
    mods = dict(model.named_modules())
    for name, m in mods.items():
        cls = type(m).__name__
        parent = type(mods[name.rsplit(".", 1)[0]]).__name__ if "." in name else ""
        if cls == "Conv":
            k, s = tuple(m.conv.kernel_size), tuple(m.conv.stride)
            if (k, s) not in (((1, 1), (1, 1)), ((3, 3), (2, 2))):
                raise ValueError("%s: a Conv the audit has no unit kind for: k %s stride %s" % (name, k, s))
            out.append(Unit(name, "conv1x1" if k == (1, 1) else "conv3x3s2", m, "silu", direct=(parent == "RepHDW" and name.endswith(".conv1"))))
        elif cls == "RepVGGBlock":
            out.append(Unit(name, "repvgg", m, "relu"))
        elif cls == "UniRepLKNetBlock":
            out.append(Unit(name, "unirep", m, "silu" if parent == "DepthBottleneckUni" else None))
        elif cls == "SPPF":
            out.append(Unit(name + ".m", "sppf_pool", m))
        elif cls == "MP":
            out.append(Unit(name, "mp", m))
        elif cls == "Head_DepthUni":
            out.append(Unit(name + ".cls_pred", "pred", m.cls_pred, direct=True))
            out.append(Unit(name + ".reg_pred", "pred", m.reg_pred, direct=True))
    return out


def in_stage(unit, stage):
    lo, hi = STAGES[stage]
    return lo <= unit.node <= hi


def predicted_pairs(us):
    """(unit, tensor) pairs the audit compares for the units `us`: y twice (in place, replay), dx once (replay), every parameter gradient twice, running_mean and running_var of every
    BatchNorm twice — from the enumeration alone"""
    return sum(2 + 1 + 2 * len(u.params) + 4 * len(u.bns) for u in us)


def read_input(x):
    """the values the unit's first kernel read, in fp64 on the CPU: the stored tensor itself; an fp32 tensor (the image) is cast to fp16 first, as autocast does in front of a convolution"""
    x = x.detach()
    if x.dtype == torch.float32:
        x = x.to(torch.float16)
    return x.double().cpu().contiguous()


def bn_batch(z, gamma, beta, eps, moments=None):
    """training-mode BatchNorm2d of z [B, C, H, W] in the dtype of z: two-pass mean and BIASED variance per channel (bn_ref.moments), or the `moments` = (mean, var) handed in —
    statistics taken somewhere else than from z, for bisecting inside a unit.  -> (out, mean, var)"""
    if moments is None:
        mean = z.mean((0, 2, 3))
        var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    else:
        mean, var = moments
    out = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return out, mean, var


def _act(u, act):
    if act == "silu":
        return u * torch.sigmoid(u)
    if act == "relu":
        return torch.clamp(u, min=0)
    return u


def forward64(unit, x, P, stats=None, moments=None, taps=None, relu_mask=None):
    """the unit's forward in the dtype of x / P (fp64 in the audit), plain torch.  P: {parameter name: tensor}.  stats (a dict): filled with {bn name: (mean, var, values per channel)}.
    moments: {bn name: (mean, var)} to normalise with instead of the batch's own.  taps (a dict): filled with the unit's inner tensors by name (unirep: "sum", the branch sum; repvgg:
    "u", the sum in front of the ReLU).  relu_mask (repvgg): u * relu_mask in place of ReLU(u) — the ReLU linearised at a mask handed in (see `reference`)."""
    m, kind = unit.module, unit.kind

    def bn(tag, z):
        mod = dict(unit.bns)[tag]
        out, mean, var = bn_batch(z, P[tag + ".weight"], P[tag + ".bias"], mod.eps, None if moments is None else moments.get(tag))
        if stats is not None:
            stats[tag] = (mean.detach(), var.detach(), z.numel() // z.shape[1])
        return out

    if kind in ("conv1x1", "conv3x3s2"):
        return _act(bn("bn", F.conv2d(x, P["conv.weight"], None, m.conv.stride, m.conv.padding)), "silu")
    if kind == "repvgg":
        u = bn("rbr_dense.bn", F.conv2d(x, P["rbr_dense.conv.weight"], None, 2, 1)) + bn("rbr_1x1.bn", F.conv2d(x, P["rbr_1x1.conv.weight"], None, 2, 0))
        if taps is not None:
            taps["u"] = u
        return _act(u, "relu") if relu_mask is None else u * relu_mask
    if kind == "unirep":
        d, c = m.dwconv, x.shape[1]
        s = bn("dwconv.origin_bn", F.conv2d(x, P["dwconv.lk_origin.weight"], None, 1, d.kernel_size // 2, 1, c))
        for kk in d.kernel_sizes:
            s = s + bn("dwconv.dil_bn_k%d_1" % kk, F.conv2d(x, P["dwconv.dil_conv_k%d_1.weight" % kk], None, 1, kk // 2, 1, c))
        if taps is not None:
            taps["sum"] = s
        return _act(bn("norm", s), unit.act)
    if kind == "sppf_pool":
        k = m.m.kernel_size
        p1 = F.max_pool2d(x, k, 1, k // 2)
        p2 = F.max_pool2d(p1, k, 1, k // 2)
        return torch.cat([p1, p2, F.max_pool2d(p2, k, 1, k // 2)], 1)
    if kind == "mp":
        return F.max_pool2d(x, 2, 2)
    if kind == "pred":
        return F.conv2d(x, P["weight"], P["bias"])
    raise ValueError(kind)


def reference(unit, x, dy, pre=None, stored_y=None):
    """{key: fp64 CPU tensor} of the unit in fp64 on its stored input x and stored upstream gradient dy.  pre: {bn name: (running_mean, running_var)} before the step — then the
    running statistics after it are among the results (momentum of the module, unbiased variance).
    stored_y (repvgg units): the output the implementation under comparison STORED.  y of the result is the plain ReLU(u) all the same; the BACKWARD is that of u * (stored_y > 0), the
    ReLU linearised where the implementation's own forward left it.  ReLU is the one discontinuous operation of the graph: whichever way a sum within an fp16 ulp of zero falls,
    the whole gradient of that output value appears or vanishes, in the framework's step as in any other, and max |got - ref| then measures which values fell which way, not arithmetic
    (tests/test_gpu_train.py::test_repvgg_block_branch_sum_with_relu_in_one_apply_pass names the same effect).  The mask is a stored tensor of the block like its input, and it is not
    taken on trust: a value whose mask differs from the fp64 one has |y - ReLU(u)| = |u| or y, so the bar on y bounds every such value to within rounding of zero."""
    x64 = read_input(x).requires_grad_()
    P = {n: p.detach().double().cpu().requires_grad_() for n, p in unit.params}
    stats, taps = {}, {}
    mask = None
    if stored_y is not None and unit.kind == "repvgg":
        mask = (stored_y.detach().double().cpu() > 0).double()
    y = forward64(unit, x64, P, stats, taps=taps, relu_mask=mask)
    if "sum" in taps:
        taps["sum"].retain_grad()
    y.backward(dy.detach().double().cpu())
    if mask is not None:
        y = _act(taps["u"], "relu")
    out = {"y": y.detach(), "dx": x64.grad}
    for n, _ in unit.params:
        out["g:" + n] = P[n].grad
    for k in cancelling_keys(unit):
        out["scale:" + k] = taps["sum"].grad.abs().sum((0, 2, 3)).max()
    if pre is not None:
        for n, mod in unit.bns:
            mean, var, M = stats[n]
            rm0, rv0 = pre[n]
            out["rm:" + n] = (1 - mod.momentum) * rm0.double().cpu() + mod.momentum * mean
            out["rv:" + n] = (1 - mod.momentum) * rv0.double().cpu() + mod.momentum * var * M / (M - 1)
    return out


def cancelling_keys(unit):
    """Tensors of a unit whose exact value is ZERO by construction: the gradient of a branch BatchNorm's bias inside a UniRepLKNetBlock.  The branch sum s = sum_j BN_j(z_j) is
    normalised by `norm` with batch statistics, which removes any per-channel constant, so d loss / d beta_j = sum over the pixels of (d loss / d s) = 0 whatever the data (the fp64
    reference gives 1e-17).  max |ref| is no scale for such a tensor; its error is measured against what the sum is made of — max over the channels of sum over the pixels of
    |d loss / d s| of the fp64 reference, the scale an implementation's rounding of the terms is proportional to (`scale:<key>` of `reference`)."""
    if unit.kind != "unirep":
        return []
    return ["g:" + n for n, _ in unit.params if n.startswith("dwconv.") and n.endswith(".bias")]          # origin_bn.bias, dil_bn_k*_1.bias (the depth-wise convs have no bias)


def run_unit(unit, x, ops):
    """the unit's own calls, alone, on the package's path (`ops`: the package's train_ops module, handed in by the caller) with out=None: what the unit runs in place — the module's
    forward, or for the `direct` units the sequence of train_ops calls the cat-free path makes"""
    m, kind = unit.module, unit.kind
    if kind in ("conv1x1", "conv3x3s2"):
        if unit.direct:
            return ops.bn_act(ops.conv1x1(x, m.conv.weight), m.bn, "silu")
        return m(x)
    if kind in ("repvgg", "mp"):
        return m(x)
    if kind == "unirep":
        return m(x, act=unit.act)
    if kind == "sppf_pool":
        k = m.m.kernel_size
        p1 = ops.maxpool_s1(x, k)
        p2 = ops.maxpool_s1(p1, k)
        return torch.cat([p1, p2, ops.maxpool_s1(p2, k)], 1)
    if kind == "pred":
        return ops.conv1x1(x, m.weight, m.bias)
    raise ValueError(kind)


def key_class(key):
    return "y" if key == "y" else "stat" if key[:3] in ("rm:", "rv:") else "grad"


def bar_a(key):
    return BAR_A[key_class(key)]


def bar_b(e_fw):
    return BAR_B_MULT * e_fw + BAR_B_ULP


def errors(got, ref, keys):
    """{key: err_max} — every reference tensor finite with max |ref| > 0 (a tensor that is identically zero would pass anything), every result finite"""
    out = {}
    for k in keys:
        r, g = ref[k], got[k].detach().double().cpu()
        scale = ref.get("scale:" + k)                            # a tensor that is zero by construction (cancelling_keys): the scale of its terms
        if not (bool(torch.isfinite(r).all()) and float(r.abs().max() if scale is None else scale) > 0):
            raise AssertionError("reference tensor %s is not finite or identically zero" % k)
        if g.shape != r.shape:
            raise AssertionError("%s: shape %s against the reference's %s" % (k, tuple(g.shape), tuple(r.shape)))
        if not bool(torch.isfinite(g).all()):
            out[k] = float("inf")
        elif scale is None:
            out[k] = bn_ref.err_max(g, r)
        else:
            out[k] = float((g - r).abs().max()) / float(scale)
    return out


def judge(e_hip, e_fw, own=None):
    """[(key, e_hip, e_fw, which bar)] of the tensors over Bar A or Bar B.  own: {key: bar} for tensors with a NAMED design difference — that bar replaces Bar B; Bar A is never relaxed."""
    bad = []
    for k, e in e_hip.items():
        if not e <= bar_a(k):
            bad.append((k, e, e_fw[k], "A"))
        elif not e <= (own[k] if own and k in own else bar_b(e_fw[k])):
            bad.append((k, e, e_fw[k], "B"))
    return bad
