"""Fingerprints of the launch plans engine.Plan builds, for tests/test_plan_identity_host.py: a change to engine.py that is meant to leave the
plans alone is checked against what the plans were BEFORE it.

    python tools/make_golden_plan.py        ->  tests/golden/plan_fingerprints.json      (run at the commit whose plans are the reference)

Plans build on torch.device("cpu") and are pure data.  Weights: synth.synth_state_dict (NumPy's legacy generator: the same bits everywhere), and
everything between them and the packed blob is element-wise.  Per plan: one digest per op over its name and every maf_op_t field, pointers
rewritten as offsets from the arena / the weight blob (a pointer into neither is an error), the arena size, the digest of the weight blob and the
digest of everything in the python-side op records that the op fields do not already cover."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import maf_yolo_amd as M  # noqa: E402
from maf_yolo_amd import lib, synth  # noqa: E402
from maf_yolo_amd.engine import Plan, Buf, Seg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")
SCALES = ("n", "s", "m")
PLAN_KW = ("fuse", "fuse_head", "fuse_tail")            # keywords of Plan(); every other setting of a case is an attribute of the model
_U8 = (2, 64, 64, lib.F16, lib.U8)
# name -> (num_classes, B, H, W, dtype, in_dtype, settings)
CASES = {
    "f16":            (80, 2, 64, 64, lib.F16, lib.F16, {}),
    "f32":            (80, 2, 64, 64, lib.F32, lib.F32, {}),
    "fuse0":          (80, *_U8, {"fuse": False}),
    "fuse1":          (80, *_U8, {"fuse": True}),
    "fuse2":          (80, *_U8, {"fuse": 2}),
    "tail1_fuse1":    (80, *_U8, {"fuse_tail": True, "fuse": True}),
    "tail0_fuse1":    (80, *_U8, {"fuse_tail": False, "fuse": True}),
    "stem0":          (80, *_U8, {"fuse_stem": False}),
    "stem1":          (80, *_U8, {"fuse_stem": 1}),
    "cat_interleaved": (80, *_U8, {"split_cat": False}),
    "lanes1":         (80, *_U8, {"multi_stream": 1}),
    "lanes2_fuse0":   (80, *_U8, {"multi_stream": 2, "fuse": False}),
    "notwin_fuse0":   (80, 2, 64, 64, lib.F16, lib.F16, {"twin_convs": False, "fuse": False}),
    "fusedict_nohead": (80, 1, 96, 160, lib.F16, lib.F32, {"fuse": {"backbone.2.m.0": 1, "backbone.4.m.0": 2}, "fuse_head": False}),
    "mprep_fuse0":    (80, 8, 384, 384, lib.F16, lib.U8, {"fuse_mprep": True, "fuse": False}),      # node 3: 18 432 output pixels, UNDER the one-launch thresholds: two launches
    "mprep":          (80, 8, 384, 384, lib.F16, lib.U8, {"fuse_mprep": True}),
    "mprep768_fuse0": (80, 8, 768, 768, lib.F16, lib.U8, {"fuse_mprep": True, "fuse": False}),      # node 3: 73 728 output pixels, over them: ONE launch (n, s: the LDS form; m: register weights)
    "mprep768":       (80, 8, 768, 768, lib.F16, lib.U8, {"fuse_mprep": True}),
    "640":            (80, 1, 640, 640, lib.F16, lib.U8, {}),
    "nc3":            (3, 2, 64, 64, lib.F16, lib.F16, {}),                                          # prediction conv padded to 4 channels, no fused head
}


def make_model(scale, nc):
    m = M.Model(scale, num_classes=nc).eval()
    m.load_state_dict(synth.synth_state_dict(m, scale, 0))
    return m


def case_args(case):
    """(B, H, W, dtype, in_dtype), the model attributes and the Plan keywords of a case."""
    _, B, H, W, dt, in_dt, settings = CASES[case]
    return (B, H, W, dt, in_dt), {k: v for k, v in settings.items() if k not in PLAN_KW}, {k: v for k, v in settings.items() if k in PLAN_KW}


def build_plan(model, case):
    """The plan of a case; the model's attributes are as they were afterwards."""
    shape, attrs, kw = case_args(case)
    missing = object()
    keep = {k: model.__dict__.get(k, missing) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        return Plan(model, *shape, torch.device("cpu"), **kw)
    finally:
        for k, v in keep.items():
            if v is missing:
                delattr(model, k)
            else:
                setattr(model, k, v)


def _digest(obj, n=16):
    return hashlib.sha256(repr(obj).encode()).hexdigest()[:n]


def _ptr(plan, v):
    v = int(v or 0)
    if v == 0:
        return 0
    if plan._abase <= v < plan._abase + plan._arena_size:
        return ("a", v - plan._abase)
    wbase = plan.weights.data_ptr()
    if wbase <= v < wbase + plan.weights.numel():
        return ("w", v - wbase)
    raise AssertionError("pointer %#x lies neither in the arena nor in the weight blob" % v)


def _field(plan, ctype, v):
    if ctype is C.c_void_p:
        return _ptr(plan, v)
    if issubclass(ctype, C.Array):
        return tuple(_field(plan, ctype._type_, e) for e in v)
    if issubclass(ctype, C.Structure):
        return tuple((n, _field(plan, t, getattr(v, n))) for n, t in ctype._fields_)
    return v


def op_fields(plan, i):
    """Op i as (name, ((field, value), ...)) with every pointer an offset from its base."""
    o = plan.ops[i]
    return plan.op_names[i], tuple((n, _field(plan, t, getattr(o, n))) for n, t in lib.MafOp._fields_)


def _plain(v):
    """A record entry without what the op fields already cover: a tensor leaves its shape and the digest of its bytes, a Buf / Seg nothing."""
    if isinstance(v, torch.Tensor):
        t = v.detach().contiguous()
        return ("T", str(t.dtype), tuple(t.shape), hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16])
    if isinstance(v, (Buf, Seg)):
        return "-"
    if isinstance(v, dict):
        return tuple((k, _plain(v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return tuple(_plain(e) for e in v)
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def weights_digest(plan):
    return hashlib.sha256(plan.weights.cpu().numpy().tobytes()).hexdigest()[:16]


def fingerprint(plan):
    return {"n_ops": len(plan.ops), "arena": plan._arena_size, "weights": weights_digest(plan),
            "records": _digest([_plain(r) for r in plan._ops]),
            "ops": [_digest(op_fields(plan, i), 12) for i in range(len(plan.ops))]}


def main():
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    plans = {}
    for scale in SCALES:
        models = {}
        for case, spec in CASES.items():
            if spec[0] not in models:
                models[spec[0]] = make_model(scale, spec[0])
            plans["%s/%s" % (scale, case)] = fingerprint(build_plan(models[spec[0]], case))
    with open(OUT, "w") as f:
        json.dump({"commit": commit, "plans": plans}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d plans, %d bytes" % (os.path.relpath(OUT, ROOT), len(plans), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
