"""-m gpu: block-local audit of ONE AMP train step (autocast fp16, scaled backward) of n, s and m in the DEFAULT mode — atomic statistics, the 1x1 conv's statistics epilogue, the merged
branch-sum BatchNorm, dw_branches with its statistics epilogue, cat-free slots — every unit of tests/amp_block_ref.py against fp64 ON THE UNIT'S OWN STORED TENSORS.

The end-to-end AMP check (tests/test_gpu_train.py::_train_step_vs_reference) compares gradients through ~150 layers of batch-statistics BatchNorm, where fp16 rounding compounds
chaotically: its bars are multiples of a parameter's largest gradient, and it runs under train_ops.set_deterministic, which turns the default composition off.  Here nothing compounds:

  capture   one hooked step (weights synth_state_dict(scale, 0), images synth_images(2, size, 7), the five labels of the end-to-end test, ComputeLoss with its own — warm-up — assigner,
            (loss * 1024).backward()).  Per unit: the input as stored, the output as stored, the gradient arriving at the output (a tensor hook: the sum over its consumers), and
            after backward the unit's parameter gradients and running statistics.  Units the cat-free path reaches without a module call (RepHDW.conv1, the prediction convs, SPPF's
            pools) are captured by wrapping train_ops.conv1x1 / bn_act / maxpool_s1 for the step.  SPPF's pools: y = cat(p1, p2, p3), dy = the channels of cv2's data gradient behind
            cv1's slot (a tensor hook on cv2's input), so the chain's own backward carries the gradient from pool to pool.
            The hooks do not change the path: the train_ops.stats deltas (native_*, fallback, torch_bn, framework_wgrad_fp32) equal those of an unhooked step on the same inputs,
            fallback == 0, loss and head outputs agree with the unhooked step's to the run-to-run spread of the atomic statistics (measured on two unhooked steps, see below) and
            bit for bit under fixed-order statistics.
  replay    every unit alone on the HIP path under the same autocast: captured input (detached, requires_grad), a pre-step copy of its parameters and running statistics, out=None,
            backward(captured dy) — the unit's own dx, and y / parameter gradients / statistics a second time.  Then the same with train_ops.framework_ops = True: torch + MIOpen on
            this GPU, the comparator of the end-to-end test.
  judge     amp_block_ref: err_max against fp64; Bar A (1e-2 / 2e-2 / 2e-3) and Bar B (e_hip <= 1.5 e_fw + 2**-10) on every tensor, in place and from the replay; the count of compared
            (unit, tensor) pairs equals the enumeration's prediction; every dy and every reference tensor finite and non-zero.

Two things the inputs above decide, stated because they bound what "every gradient is non-zero" can mean (tests/test_amp_block_host.py shows both on the CPU):
  * the box branch (reg_conv, reg_conv_s, reg_pred) of a head on whose level the assigner puts no foreground anchor receives an exactly zero gradient — the box losses are sums over
    foreground anchors.  With these labels that is the stride-32 head at 128 x 128 (n, s, m), no head at 192 x 192.  The audit asserts that rule on the device's own assignment (zero dy
    <=> box branch of a level without foreground), checks y and the statistics of those units in place, requires their in-place gradients to be EXACTLY zero, and replays them with a
    stand-in dy (seeded Gaussian, its largest value about that of the class branch's dy at the same unit) so that their backward kernels are compared at these shapes all the same;
  * the gradient of a branch BatchNorm's bias inside a UniRepLKNetBlock is zero by construction (`norm` removes the constant): measured against the scale of its terms
    (amp_block_ref.cancelling_keys).

  * ReLU (RepVGGBlock) is the one discontinuity of the graph.  Against the PLAIN fp64 ReLU backward the worst gradient error of a RepVGG unit was anywhere between 4e-4 and 0.3
    of max |g| — for the framework's ops exactly as for the kernels (n/128 backbone.1: in place 5.8e-2, replay 1.4e-1, framework 3.1e-1; m/128 backbone.7.conv2: 1.2e-1 all three;
    n/128 backbone.7.conv2: 4.4e-4 / 5.6e-4 / 6.0e-4), decided by which output values within an fp16 ulp of zero fell which way, not by arithmetic.  Each implementation's
    backward is therefore held against fp64 linearised at ITS OWN stored output's sign (amp_block_ref.reference(stored_y=)); the bar on y bounds every value whose sign differs from
    the fp64 one to within rounding of zero.  Same Bars A and B; the plain figures are printed with each RepVGG line.

The path check, as measured: with fixed-order statistics the hooked step is bit-identical to the unhooked one (loss, class scores, box logits).  With atomics two UNHOOKED steps on the
same inputs differ by |d loss| 2e-4 / 1e-4 / 6e-4, max |d cls| 3e-4 / 9e-4 / 5e-3, max |d reg| 2.6e-2 / 9.8e-2 / 0.60 (n / s / m; max |reg| 3.3 / 2.9 / 3.5), and the hooked step
differs from an unhooked one by as much (2.3e-2 / 0.12 / 0.49 in reg): rtol 2e-3 / atol 1e-3 alone holds for the class scores of n and s only, so the tolerance is that plus twice
the spread of the two unhooked steps.  The path counters are equal in every case, fallback = torch_bn = glue = 0.

MEASURED (one run on the MI355X; ratio = e_hip / max(e_fw, 2**-10), e_hip the larger of in place and replay; every run reorders the atomics, so the third digit moves):

  EVERY unit of n, s and m is inside Bar A and Bar B: 0 of 1 668 (n/128), 1 668 (n/192), 2 368 (s/128), 3 058 (m/128: 1 091 + 1 542 + 425) and 1 668 (n/128, fixed order) pairs over.
  m's end-to-end 2.36 x (VERDICT weak #2) is therefore the amplification of correct local results, not a lossy kernel.

  worst ratio per unit kind      n/128   n/192   s/128   m/128   n/128 fixed order
    conv1x1                      1.44    1.20    1.30    1.11    1.28      (always a BatchNorm weight's gradient, e_hip 1.7e-3 ... 4.1e-3 against e_fw 1.3e-3 ... 3.4e-3)
    conv3x3s2                    0.63    0.64    0.64    0.69    0.88
    repvgg                       0.69    0.72    1.00    0.73    0.77
    unirep                       1.50    1.04    1.17    1.36    1.31      (n/128: backbone.33.reg_conv g:dwconv.dil_conv_k7_1.weight 2.6e-3 against 1.7e-3: under Bar B's 3.5e-3)
    sppf_pool                    0.55    0.79    0.66    0.55    0.76      (y exact; dx = the framework's to the last digit)
    mp                           0.00    0.00    0.00    0.00    0.00      (exact)
    pred                         0.57    0.61    0.61    0.48    0.60
  the five worst units of m      backbone.2.m.1.conv2 (unirep, 2 x 144 x 32 x 32) 1.36; backbone.30.m.0.conv2 (unirep, 2 x 576 x 4 x 4) 1.24; backbone.33.reg_conv (unirep, 2 x 384 x 4 x 4,
                                 stand-in dy) 1.24; backbone.30.m.1.conv2 (unirep) 1.20; backbone.4.m.2.conv1 (conv1x1, 2 x 96 x 16 x 16) 1.11
  largest errors over m          y 1.4e-3, dx 3.3e-3, a parameter gradient 4.7e-3, a running statistic 1.3e-4 (framework on the same tensors: 4.7e-3, 5.3e-3, 7.3e-3, 3.7e-4)
  wall time of the file          42.6 s: captures + replays 12.8 s (n/128, the process's first: the conv tuner times its candidates), 7.3 s (n/192), 4.8 s (s), 5.6 s (m), 0.7 s (n fixed
                                 order); the fp64 references 1.0 / 1.4 / 2.0 / 4.0 (m: 1.5 + 2.1 + 0.4) / 1.0 s
"""
import os
import time

import pytest
import torch

import maf_yolo_amd as M
from maf_yolo_amd import train_ops
from oracle import maf_oracle as O

import amp_block_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16 = torch.float16

_TARGETS = [[0, 3, 0.40, 0.50, 0.30, 0.40], [0, 17, 0.70, 0.30, 0.20, 0.50], [0, 17, 0.25, 0.75, 0.30, 0.25],
            [1, 5, 0.50, 0.50, 0.60, 0.60], [1, 62, 0.20, 0.30, 0.25, 0.35]]          # tests/test_gpu_train.py::_TRAIN_TARGETS (normalised: ComputeLoss scales them to the image)

# Units with a NAMED design difference: (scale, size, deterministic, unit, "in place" | "replay", key) -> its own bar in place of Bar B, 1.25 x the measured e_hip (Bar A is never relaxed)
OWN_BARS = {}


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                  # a fault of the device: nothing more is started on it
        pytest.exit("the device reported %s after %s: stopping" % (e, what), returncode=3)


def _model(scale):
    m = M.Model(scale)
    m.load_state_dict(O.synth_state_dict(scale, 0))
    return m.to(DEV).train()


def _path_key(k):
    return k.startswith("native_") or k in ("fallback", "torch_bn", "framework_wgrad_fp32", "glue", "conv_bn_stats", "bn_sum_next_stats", "cat_free", "cat_copied_parts")


def _step(m, x, targets, size):
    """one AMP train step -> (loss, cls, reg, path counters, own assignment [B, A], map sizes per level)"""
    crit = M.ComputeLoss(ori_img_size=size)                    # the reference's defaults: the warm-up assigner at epoch 0
    n0 = dict(train_ops.stats)
    with torch.autocast("cuda", dtype=F16):
        (feats, cls, reg), _ = m(x)
    loss, _ = crit((feats, cls, reg), targets, 0, 1)
    (loss * 1024.0).backward()
    _sync("a train step")
    d = {k: train_ops.stats.get(k, 0) - n0.get(k, 0) for k in set(train_ops.stats) | set(n0) if _path_key(k)}
    return loss.detach().float(), cls.detach().float().clone(), reg.detach().float().clone(), d, crit.last_assignment[0].clone(), [tuple(f.shape[-2:]) for f in feats]


def _hooked_step(m, us, x, targets, size):
    """the step with every unit's stored input, stored output and arriving gradient recorded: {unit name: {x, y, dy}}"""
    cap, handles, pend, pools, cat_grad = {}, [], {}, [], []

    def rec(u, xin, out):
        assert u.name not in cap, "%s was captured twice" % u.name
        c = cap[u.name] = {"x": xin.detach().clone(), "y": out.detach().clone(), "via": "call"}

        def on_grad(g):
            assert "dy" not in c, "%s: a second gradient arrived at the output" % u.name
            c["dy"] = g.detach().clone()
        out.register_hook(on_grad)
        return c

    def module_hook(u):
        def h(mod, args, kwargs, out):
            if u.kind == "unirep":
                assert kwargs.get("act") == u.act, (u.name, kwargs)
            rec(u, args[0], out)["via"] = "module"
        return h

    by_weight, by_bn = {}, {}
    sppf = None
    for u in us:
        if u.kind == "pred":
            by_weight[id(u.module.weight)] = u
        elif u.kind == "sppf_pool":
            sppf = u
            handles.append(u.module.cv2.register_forward_pre_hook(lambda mod, args, kwargs: args[0].register_hook(lambda g: cat_grad.append(g.detach().clone())) and None, with_kwargs=True))
        else:
            handles.append(u.module.register_forward_hook(module_hook(u), with_kwargs=True))
            if u.direct:
                by_weight[id(u.module.conv.weight)], by_bn[id(u.module.bn)] = u, u
    orig = (train_ops.conv1x1, train_ops.bn_act, train_ops.maxpool_s1)

    def conv1x1(xin, w, bias=None):
        out = orig[0](xin, w, bias)
        u = by_weight.get(id(w))
        if u is not None and u.kind == "pred":
            rec(u, xin, out)
        elif u is not None:
            pend[u.name] = xin                                   # RepHDW.conv1: the BatchNorm call behind it completes the unit
        return out

    def bn_act(z, bn, act=None, residual=None, pre_stats=None, out=None):
        y = orig[1](z, bn, act, residual=residual, pre_stats=pre_stats, out=out)
        u = by_bn.get(id(bn))
        if u is not None and u.name in pend:
            assert act == "silu" and residual is None
            rec(u, pend.pop(u.name), y)
        return y

    def maxpool_s1(xin, k, out=None):
        y = orig[2](xin, k, out=out)
        pools.append((xin.detach().clone(), y.detach().clone()))
        return y

    train_ops.conv1x1, train_ops.bn_act, train_ops.maxpool_s1 = conv1x1, bn_act, maxpool_s1
    try:
        res = _step(m, x, targets, size)
    finally:
        train_ops.conv1x1, train_ops.bn_act, train_ops.maxpool_s1 = orig
        for h in handles:
            h.remove()
    assert not pend, pend
    assert len(pools) == 3 and len(cat_grad) == 1, (len(pools), len(cat_grad))
    c = pools[0][1].shape[1]
    assert torch.equal(pools[1][0], pools[0][1]) and torch.equal(pools[2][0], pools[1][1]) and cat_grad[0].shape[1] == 4 * c
    cap[sppf.name] = {"x": pools[0][0], "y": torch.cat([p[1] for p in pools], 1), "dy": cat_grad[0][:, c:].clone(), "via": "call"}
    for u in us:
        assert u.name in cap and "dy" in cap[u.name], "%s was not captured" % u.name
        assert (cap[u.name]["via"] == "call") == (u.direct or u.kind == "sppf_pool"), (u.name, cap[u.name]["via"])      # `direct` is what the step did
    return cap, res


def _results(u, y, dx):
    out = {"y": y.detach().clone()}
    if dx is not None:
        out["dx"] = dx.detach().clone()
    for n, p in u.params:
        assert p.grad is not None, (u.name, n)
        out["g:" + n] = p.grad.detach().clone()
    for n, b in u.bns:
        out["rm:" + n], out["rv:" + n] = b.running_mean.detach().clone(), b.running_var.detach().clone()
    return out


def _replay(u, x, dy, pre, framework):
    """unit u of the replay model alone: pre-step running statistics, no gradients yet, out=None, backward(dy)"""
    with torch.no_grad():
        for n, b in u.bns:
            b.running_mean.copy_(pre[n][0])
            b.running_var.copy_(pre[n][1])
    for _, p in u.params:
        p.grad = None
    xin = x.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_()
    train_ops.framework_ops = framework
    try:
        with torch.autocast("cuda", dtype=F16):
            y = R.run_unit(u, xin, train_ops)
        y.backward(dy.to(y.dtype).contiguous(memory_format=torch.channels_last))
        _sync("the replay of %s (%s)" % (u.name, "framework" if framework else "HIP"))
    finally:
        train_ops.framework_ops = False
    return _results(u, y, xin.grad)


def _audit(scale, size, det=False):
    """capture + replays of one (scale, size): everything the comparisons need, on the device"""
    t0 = time.time()
    x = O.synth_images(2, size, 7).to(DEV)
    targets = torch.tensor(_TARGETS, dtype=torch.float32, device=DEV)
    tag = "%s/%d%s" % (scale, size, "/det" if det else "")
    if det:
        train_ops.set_deterministic(True)
    try:
        plain = _step(_model(scale), x, targets, size)
        again = _step(_model(scale), x, targets, size)          # a second unhooked step: what two runs of the SAME step differ by (the atomics' arrival order)
        m = _model(scale)
        us = R.units(m)
        cap, hooked = _hooked_step(m, us, x, targets, size)
        # the hooks did not change the path
        dev = [float((hooked[i] - plain[i]).abs().max()) for i in range(3)]
        spread = [float((again[i] - plain[i]).abs().max()) for i in range(3)]
        print("AMPBLK %s path: counters %s | hooked vs unhooked step: |d loss| %.2e, max |d cls| %.2e, max |d reg| %.2e | unhooked vs unhooked: %.2e, %.2e, %.2e (loss %.4f, max |reg| %.2f)"
              % ((tag, sorted(hooked[3].items())) + tuple(dev) + tuple(spread) + (float(plain[0]), float(plain[2].abs().max()))))
        assert hooked[3] == plain[3] == again[3], (hooked[3], plain[3], again[3])
        assert hooked[3].get("fallback", 0) == 0 and hooked[3].get("torch_bn", 0) == 0 and hooked[3].get("framework_wgrad_fp32", 0) == 0, hooked[3]
        # the default composition ran (merged branch sums, statistics out of the conv's and the branch sum's epilogues, cat-free slots) — none of it in the deterministic mode
        # (how many 1x1 convs carry the statistics epilogue is the tuner's choice per shape: the count is in the printed counters)
        assert (hooked[3].get("native_bn_sum", 0) > 0) == (not det), hooked[3]
        assert not det or (hooked[3].get("conv_bn_stats", 0) == 0 and hooked[3].get("bn_sum_next_stats", 0) == 0), hooked[3]
        assert hooked[3].get("cat_free", 0) > 0, hooked[3]
        # loss and head outputs: those of the unhooked step, to the run-to-run spread of the atomic statistics — rtol 2e-3 / atol 1e-3 as test_weight_staging_plan_matches_per_layer_packing
        # allows for the class scores of n, plus twice what the two UNHOOKED steps above differ by (never the hooked one): the box logits move by 2-3e-2 from run to run on n and by up
        # to 0.7 on m, through ~150 layers of fp16 and batch statistics over as few as 32 values — the chaos this audit exists to get out of the way.  With fixed-order statistics there
        # is no spread and the hooked step must be BIT-IDENTICAL to the unhooked one.
        for i, what in enumerate(("loss", "cls", "reg")):
            if det:
                assert torch.equal(hooked[i], plain[i]) and torch.equal(again[i], plain[i]), what
            else:
                assert bool(((hooked[i] - plain[i]).abs() <= 2e-3 * plain[i].abs() + 1e-3 + 2 * spread[i]).all()), (what, dev[i], spread[i])
        # levels without a foreground anchor: their box branch gets an exactly zero gradient — and nothing else does
        own_gt, hw = hooked[4], hooked[5]
        heads = [u.name.rsplit(".", 1)[0] for u in us if u.name.endswith(".cls_pred")]
        a0, nofg = 0, set()
        for head, (h, w) in zip(heads, hw):
            if int((own_gt[:, a0:a0 + h * w] >= 0).sum()) == 0:
                nofg.add(head)
            a0 += h * w
        dead = set()
        for u in us:
            dy = cap[u.name]["dy"]
            assert bool(torch.isfinite(dy).all()), "%s: the captured dy is not finite" % u.name
            is_dead = float(dy.abs().max()) == 0.0
            allowed = ".reg_" in u.name and u.name.split(".reg_")[0] in nofg
            assert is_dead == allowed, "%s: dy is %s, foreground-free heads %s" % (u.name, "all zero" if is_dead else "non-zero", sorted(nofg))
            if is_dead:
                dead.add(u.name)
        inplace = {u.name: _results(u, cap[u.name]["y"], None) for u in us}
        # replays on a model of the pre-step weights and statistics
        rmod = _model(scale)
        rus = R.units(rmod)
        assert [u.name for u in rus] == [u.name for u in us]
        pre = {u.name: {n: (b.running_mean.detach().clone(), b.running_var.detach().clone()) for n, b in u.bns} for u in rus}
        train_ops.begin_step(None, DEV)                        # no staging plan: the replayed layers pack their own weights
        hip, fw = {}, {}
        g = torch.Generator().manual_seed(17)
        for u in rus:
            c = cap[u.name]
            c["dy_replay"] = c["dy"]
            if u.name in dead:
                sib = float(cap[u.name.replace(".reg_", ".cls_")]["dy"].abs().max())
                c["dy_replay"] = (torch.randn(c["dy"].shape, generator=g) * (sib / 4)).to(F16).to(DEV)       # 4 sigma of a Gaussian: its largest value is about the class branch's
            hip[u.name] = _replay(u, c["x"], c["dy_replay"], pre[u.name], False)
            fw[u.name] = _replay(u, c["x"], c["dy_replay"], pre[u.name], True)
    finally:
        train_ops.framework_ops = False
        if det:
            train_ops.set_deterministic(False)
    print("AMPBLK %s captured and replayed %d units (%d with a stand-in dy: %s) in %.1f s" % (tag, len(us), len(dead), sorted(dead), time.time() - t0))
    return dict(tag=tag, key=(scale, size, det), units=rus, cap=cap, inplace=inplace, hip=hip, fw=fw, pre=pre, dead=dead)


@pytest.fixture(scope="module")
def audits():
    cache = {}

    def get(scale, size, det=False):
        k = (scale, size, det)
        if k not in cache:
            cache[k] = _audit(scale, size, det)
        return cache[k]
    return get


def _ratio(e, f):
    return e / max(f, R.BAR_B_ULP)


def _compare(au, stage=None):
    """every (unit, tensor) pair of the stage against fp64 under Bars A and B; prints one line per unit when something is over a bar or MAF_TEST_VERBOSE is set"""
    t0 = time.time()
    us = [u for u in au["units"] if stage is None or R.in_stage(u, stage)]
    assert us
    lines, bad, pairs, worst = [], [], 0, {}
    for u in us:
        c = au["cap"][u.name]
        got = au["inplace"][u.name]
        ref = R.reference(u, c["x"], c["dy_replay"], au["pre"][u.name])
        note = ""
        if u.kind == "repvgg":
            # ReLU: every implementation's backward against the fp64 backward linearised at ITS OWN stored output's sign (amp_block_ref.reference); the plain figures are printed
            plain = (R.errors(got, ref, u.keys(False)), R.errors(au["hip"][u.name], ref, u.keys(True)), R.errors(au["fw"][u.name], ref, u.keys(True)))
            note = " | against the plain ReLU backward: worst gradient error in place %.1e, replay %.1e, framework %.1e" % tuple(max(v for k, v in e.items() if R.key_class(k) == "grad") for e in plain)
            ref_in, ref_fw = R.reference(u, c["x"], c["dy_replay"], au["pre"][u.name], stored_y=got["y"]), R.reference(u, c["x"], c["dy_replay"], au["pre"][u.name], stored_y=au["fw"][u.name]["y"])
            ref = R.reference(u, c["x"], c["dy_replay"], au["pre"][u.name], stored_y=au["hip"][u.name]["y"])
        else:
            ref_in = ref_fw = ref
        e_fw = R.errors(au["fw"][u.name], ref_fw, u.keys(True))
        e_rep = R.errors(au["hip"][u.name], ref, u.keys(True))
        ref = ref_in
        if u.name in au["dead"]:
            # no gradient reached the unit in place: y and the statistics are compared, the gradients must be exactly zero (the replay compares them under the stand-in dy)
            e_in = R.errors(got, ref, [k for k in u.keys(False) if R.key_class(k) != "grad"])
            for k in u.keys(False):
                if R.key_class(k) == "grad":
                    e_in[k] = 0.0 if float(got[k].abs().max()) == 0.0 else float("inf")
        else:
            e_in = R.errors(got, ref, u.keys(False))
        assert list(e_in) and set(e_in) == set(u.keys(False)) and set(e_rep) == set(u.keys(True))
        pairs += len(e_in) + len(e_rep)
        own = {w: {k_[5]: v for k_, v in OWN_BARS.items() if k_[:4] == au["key"] + (u.name,) and k_[4] == w} for w in ("in place", "replay")}
        bad += [(u.name, "in place") + b for b in R.judge(e_in, e_fw, own["in place"])] + [(u.name, "replay") + b for b in R.judge(e_rep, e_fw, own["replay"])]
        cells = []
        for k in u.keys(True):
            eh = max(e_rep[k], e_in.get(k, 0.0))
            r = _ratio(eh, e_fw[k])
            cells.append("%s %s/%.1e/%.1e (%.2f)" % (k, "%.1e" % e_in[k] if k in e_in else "-", e_rep[k], e_fw[k], r))
            w = worst.get(u.kind)
            if w is None or r > w[0]:
                worst[u.kind] = (r, u.name, k, eh, e_fw[k])
        shp = tuple(c["x"].shape)
        lines.append((max(_ratio(max(e_rep[k], e_in.get(k, 0.0)), e_fw[k]) for k in e_rep),
                      "AMPBLK %s %s %s %dx%dx%dx%d | key in-place/replay/framework (ratio) | %s" % (au["tag"], u.name, u.kind, shp[0], shp[1], shp[2], shp[3], " | ".join(cells) + note)))
    if bad or os.environ.get("MAF_TEST_VERBOSE"):
        for _, ln in lines:
            print(ln)
    for kind, w in sorted(worst.items()):
        print("AMPSUM %s %s %s: worst ratio %.2f (%s %s: e_hip %.2e, e_fw %.2e)" % ((au["tag"], stage or "all", kind) + w))
    for r, ln in sorted(lines, reverse=True)[:5]:
        print("AMPTOP %s %s: %.2f %s" % (au["tag"], stage or "all", r, ln.split(" | ")[0].split(" ", 2)[2]))
    print("AMPBLK %s %s: %d units, %d (unit, tensor) pairs against fp64 in %.1f s, %d over a bar" % (au["tag"], stage or "all", len(us), pairs, time.time() - t0, len(bad)))
    assert pairs == R.predicted_pairs(us), (pairs, R.predicted_pairs(us))
    assert not bad, bad


@pytest.mark.parametrize("size", [128, 192])
def test_amp_blocks_of_n(audits, size):
    """n: 16^2 / 8^2 / 4^2 maps (the small-map dispatch) and 24^2 / 12^2 / 6^2 (ragged against 16-wide tiles and 8-row bands)"""
    _compare(audits("n", size))


def test_amp_blocks_of_s(audits):
    _compare(audits("s", 128))


@pytest.mark.parametrize("stage", ["backbone", "neck", "heads"])
def test_amp_blocks_of_m(audits, stage):
    """m, captured once, compared by stage (nodes 0-8, 9-30, 31 and up: the ranges of the end-to-end test)"""
    _compare(audits("m", 128), stage)


def test_amp_blocks_of_n_with_fixed_order_statistics(audits):
    """the mode the end-to-end AMP test runs in (train_ops.set_deterministic): the unmerged branch sums with the stand-alone statistics kernel"""
    _compare(audits("n", 128, True))
