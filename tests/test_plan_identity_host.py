"""CPU: the launch plans are what they were at the commit tests/golden/plan_fingerprints.json names, bit for bit (tools/make_golden_plan.py:
the cases, the weights and what a fingerprint holds), and Model.plan_key tells apart every setting that changes a plan.

Arena offsets follow the order of Plan._alloc calls and weight-blob offsets the order of Plan._wput calls, so equal fingerprints mean equal launch
arguments relative to the two bases: a change to engine.py that passes here hands the kernels what they were handed before."""
import importlib.util
import json
import os

import pytest
import torch

from maf_yolo_amd import lib
from maf_yolo_amd.engine import plan_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_plan", os.path.join(ROOT, "tools", "make_golden_plan.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.OUT) as _f:
    GOLDEN = json.load(_f)["plans"]


@pytest.fixture(scope="module")
def models():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    cache = {}

    def get(scale, nc=80):
        if (scale, nc) not in cache:
            cache[scale, nc] = G.make_model(scale, nc)
        return cache[scale, nc]
    return get


def test_golden_file_covers_every_case():
    assert set(GOLDEN) == {"%s/%s" % (s, c) for s in G.SCALES for c in G.CASES}
    assert os.path.getsize(G.OUT) < 100 * 1024


def paths(plan):
    """The forms the emitters can take that this plan's records show."""
    p = set()
    for r in plan._ops:
        k, n = r["kind"], r["name"]
        if "pool1" in r:
            p.add("mprep_wreg" if r.get("pool1_tk") == lib.CONV3_WREG else "mprep_lds" if "pool1_tk" not in r else "mprep_?")
        if "twin" in r:
            p.add("twin")
        if k == lib.OP_STEM:
            p.add("stem")
        if k == lib.OP_STEM2:
            p.add("stem3_split" if "out2" in r else "stem3" if "c3" in r else "stem2")
        if k == lib.OP_BOTTLENECK:
            p.add("tail" if "tail_c3" in r else "mode1")
        if k == lib.OP_CONV1DW:
            p.add("mode2")
        if k == lib.OP_DWCONV and ".m." in n:
            p.add("mode0")
        if k == lib.OP_HEADTAIL:
            p.add("headtail256" if r["Cin"] == 256 else "headtail")
        if k == lib.OP_DECODE:
            p.add("decode")
        if k == lib.OP_DWCONV and n.endswith(".cls_conv"):
            p.add("head_dw_apart")
        if k == lib.OP_DWCONV and n.endswith(".cls_reg_conv") and not any(q["kind"] == lib.OP_HEADTAIL and q["node"] == r["node"] for q in plan._ops):
            p.add("head_dw_shared")
        if r["lane"]:
            p.add("lanes")
        if r.get("out_f32") and r["Cout"] == 4:
            p.add("pred_padded")
    return p


_MPREP = {"mprep_lds", "mprep_wreg", "mprep_?"}
_MPREP768 = {"n": {"mprep_lds"}, "s": {"mprep_lds"}, "m": {"mprep_wreg"}}
# case -> (forms its plan must show, forms it must not show); a dict is per scale.  The matrix is there to take these paths: a case that stops taking
# its path (a threshold moved, a default changed) would leave the fingerprints equal and the path unchecked
PATHS = {
    "f16":             ({"n": {"stem3_split", "twin", "tail", "headtail", "mode0"}, "s": {"stem3_split", "twin", "headtail", "headtail256", "mode1"},
                        "m": {"stem3_split", "twin", "headtail256", "head_dw_shared", "decode"}}, _MPREP),
    "f32":             ({"stem", "head_dw_apart", "decode", "mode0", "twin"}, {"headtail", "headtail256", "mode1", "mode2", "tail", "stem2", "stem3", "stem3_split"}),
    "fuse0":           ({"mode0"}, {"mode1", "mode2", "tail"}),
    "fuse1":           ({"mode1", "mode2"}, {"mode0"}),
    "fuse2":           ({"mode2"}, {"mode0", "mode1", "tail"}),
    "tail1_fuse1":     ({"tail", "mode1"}, set()),
    "tail0_fuse1":     ({"mode1"}, {"tail"}),
    "stem0":           ({"stem"}, {"stem2", "stem3", "stem3_split"}),
    "stem1":           ({"stem2"}, {"stem", "stem3", "stem3_split"}),
    "cat_interleaved": ({"stem3"}, {"stem3_split"}),
    "lanes1":          ({"lanes", "head_dw_shared", "decode"}, {"twin", "headtail", "headtail256"}),
    "lanes2_fuse0":    ({"lanes", "head_dw_shared", "decode"}, {"twin", "headtail", "headtail256"}),
    "notwin_fuse0":    ({"mode0"}, {"twin"}),
    "fusedict_nohead": ({"mode2", "head_dw_shared", "decode"}, {"headtail", "headtail256"}),
    "mprep_fuse0":     ({"mode0"}, _MPREP),                       # 18 432 output pixels at node 3: under the one-launch thresholds
    "mprep":           ({"twin"}, _MPREP),
    "mprep768_fuse0":  (_MPREP768, {"mode1", "mode2", "tail"}),
    "mprep768":        (_MPREP768, set()),
    "640":             ({"twin", "stem3_split"}, _MPREP),
    "nc3":             ({"pred_padded", "head_dw_shared", "decode"}, {"headtail", "headtail256"}),
}


@pytest.mark.parametrize("case", list(G.CASES))
@pytest.mark.parametrize("scale", G.SCALES)
def test_plan_is_the_recorded_one(models, scale, case):
    model = models(scale, G.CASES[case][0])
    plan = G.build_plan(model, case)
    want, never = (v[scale] if isinstance(v, dict) else v for v in PATHS[case])
    assert want <= paths(plan) and not never & paths(plan), (sorted(paths(plan)), sorted(want), sorted(never))
    got, want = G.fingerprint(plan), GOLDEN["%s/%s" % (scale, case)]
    assert got["n_ops"] == want["n_ops"], plan.op_names
    first = next((i for i, (a, b) in enumerate(zip(got["ops"], want["ops"])) if a != b), None)
    assert first is None, "first op that differs: %d %s %r" % (first, plan.op_names[first], G.op_fields(plan, first))
    assert got == want, {k: (got[k], want[k]) for k in ("arena", "weights", "records") if got[k] != want[k]}
    # the options the plan was built from are the ones the cache key of the same settings holds
    # (Model.plan_for hands Plan fuse_head and, under autotune, the modes choose_fusion measured — no case here — and no other keyword: there the same
    # settings are attributes of the model)
    (B, H, W, dt, in_dt), attrs, kw = G.case_args(case)
    attrs = dict(attrs, **{{"fuse": "fuse_bottlenecks"}.get(k, k): v for k, v in kw.items()})
    keep = {k: model.__dict__.get(k, KeyError) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        assert plan.options == plan_options(model, dt, None, bool(model.fuse_head), None)
        in_key = plan.options._replace(fuse=repr(plan.options.fuse)) if isinstance(plan.options.fuse, dict) else plan.options
        assert in_key in model.plan_key((B, H, W), dt, in_dt, None)
    finally:
        for k, v in keep.items():
            delattr(model, k) if v is KeyError else setattr(model, k, v)
    for name in plan.options._fields:
        assert getattr(plan, name) == getattr(plan.options, name), name


def test_fingerprint_sees_a_change(models):
    plan = G.build_plan(models("n"), "f16")
    base = G.fingerprint(plan)
    i = next(i for i, o in enumerate(plan.ops) if o.kind == lib.OP_CONV1X1)
    for field in ("tile_c", "out_coff"):
        old = getattr(plan.ops[i], field)
        setattr(plan.ops[i], field, old + 8)
        ops = G.fingerprint(plan)["ops"]
        setattr(plan.ops[i], field, old)
        assert [j for j, (a, b) in enumerate(zip(ops, base["ops"])) if a != b] == [i], field
    assert G.fingerprint(plan) == base
    plan.weights[plan.weights.numel() // 2] ^= 1
    assert G.weights_digest(plan) != base["weights"]
    plan.ops[i].out = plan._abase + plan._arena_size + 4096          # a pointer into neither range
    with pytest.raises(AssertionError):
        G.fingerprint(plan)


# ---------------------------------------------------------------- Model.plan_key (no GPU tensor needed)
def _key(m, head_feats=False, slot=0):
    return m.plan_key((2, 64, 64), lib.F16, lib.U8, 0, head_feats, slot)


def test_plan_key_is_equal_for_equal_settings(models):
    m = models("n")
    assert _key(m) == _key(m) and hash(_key(m)) == hash(_key(m))
    m.fuse_bottlenecks = {"backbone.2.m.0": 1}                       # an unhashable setting enters by its repr
    try:
        assert _key(m) == _key(m) and hash(_key(m)) == hash(_key(m))
    finally:
        m.fuse_bottlenecks = "auto"


@pytest.mark.parametrize("attr,value", [("fuse_mprep", True), ("split_cat", False), ("autotune", True), ("fuse_stem", 1), ("fuse_stem", False),
                                        ("fuse_bottlenecks", False), ("fuse_bottlenecks", {"backbone.2.m.0": 1}), ("fuse_tail", True), ("fuse_tail", False),
                                        ("multi_stream", 1), ("multi_stream", 2), ("twin_convs", False), ("fuse_head", False)])
def test_plan_key_changes_with_each_setting(models, attr, value):
    m = models("n")
    base = _key(m)
    keep = m.__dict__.get(attr, KeyError)
    setattr(m, attr, value)
    try:
        assert _key(m) != base
    finally:
        delattr(m, attr) if keep is KeyError else setattr(m, attr, keep)
    assert _key(m) == base


def test_plan_key_changes_with_head_feats_slot_shape_and_dtypes(models):
    m = models("n")
    base = _key(m)
    assert _key(m, head_feats=True) != base and _key(m, slot=1) != base
    assert m.plan_key((1, 64, 64), lib.F16, lib.U8, 0) != base and m.plan_key((2, 64, 64), lib.F32, lib.U8, 0) != base
    assert m.plan_key((2, 64, 64), lib.F16, lib.F16, 0) != base and m.plan_key((2, 64, 64), lib.F16, lib.U8, 1) != base
