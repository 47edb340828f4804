"""-m gpu: whole-path parity of Model.forward() + non_max_suppression() on the HIP engine.

* fp32 engine vs the golden fixtures the REFERENCE produced (tests/golden/, tools/make_golden.py) and
  vs the oracle on fresh seeded inputs: boxes |d| <= 1e-3 + 1e-5*|ref| px, scores 2e-5
  (north_star: "within 1e-3 fp32"; the relative term covers box coordinates ~1e3 px where one
  fp32 ulp is 6e-5).
* fp16 engine (the metric's configuration: fp16 storage, fp32 accumulate) vs the same fp32 golden:
  twice the gap measured on the device (tools/fp16_gap.py, round 2): n / s: boxes 0.3 px + 0.5 %, scores
  2e-3 / 5e-3; m (deepest graph, 151 convs of fp16 rounding): boxes 2.2 px + 0.5 %, scores 9e-3.  The gap is
  fp16 storage of the activations, not kernel error: the same kernels in fp32 mode meet 1e-3, and every
  fused fp16 kernel is held to 2e-3 against an fp32 reference with the same rounding points
  (tests/test_gpu_fused_parity.py, tests/test_gpu_kernels.py).
* NMS: rows AND flat survivor indices identical to the oracle / golden (bit-exact).
"""
import numpy as np
import pytest
import torch

import maf_yolo_amd as M
import nms_cases
from oracle import maf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _close32(pred, ref):
    np.testing.assert_allclose(pred[..., :4], ref[..., :4], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(pred[..., 4:], ref[..., 4:], rtol=0, atol=2e-5)


_TOL16 = {"n": (0.3, 2e-3), "s": (0.5, 5e-3), "m": (2.2, 9e-3)}     # (box atol in px at rtol 5e-3, score atol): 2x the measured fp16-vs-fp32 gap


def _close16(pred, ref, scale="n"):
    box_atol, score_atol = _TOL16[scale]
    np.testing.assert_allclose(pred[..., :4], ref[..., :4], rtol=5e-3, atol=box_atol)
    np.testing.assert_allclose(pred[..., 4:], ref[..., 4:], rtol=0, atol=score_atol)


@pytest.fixture(scope="module")
def models():
    out = {}
    for s in "nsm":
        m = M.Model(s)
        m.load_state_dict(O.synth_state_dict(s, 0))
        out[s] = m.to(DEV).eval()
    return out


@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_forward_320_vs_reference_golden(golden, models, scale):
    g = golden("maf_" + scale)
    x = O.synth_images(1, 320, 1).to(DEV)
    with torch.no_grad():
        p32, feats = models[scale](x)
        p16 = models[scale](x.half())[0]
    assert p32.shape == (1, 2100, 85) and p32.dtype == torch.float32 and len(feats) == 3
    _close32(p32.cpu().numpy(), g["pred320_deploy"])
    _close16(p16.cpu().numpy(), g["pred320_deploy"], scale)
    # featmaps: (stem, cls, reg) NCHW like the reference's second return value
    t, cls, reg = feats[2]
    assert cls.shape == (1, 80, 10, 10) and reg.shape == (1, 68, 10, 10)
    np.testing.assert_allclose(cls.float().cpu().numpy(), g["head2_cls"], atol=2e-5)
    np.testing.assert_allclose(reg.float().cpu().numpy(), g["head2_reg"], rtol=1e-4, atol=2e-4)


def test_per_node_taps_vs_reference(golden, models):
    """Every materialised node output of the fp32 plan equals the reference's forward-hook capture (64x64)."""
    g = golden("maf_n")
    m = models["n"]
    x = O.synth_images(1, 64, 2).to(DEV)
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    plan = m.plan_for(x)
    last = {}                                   # node -> (last op of that node, address of its output buffer)
    for o, name in zip(plan.ops, plan.op_names):
        if name.startswith("backbone."):
            last[int(name.split(".")[1])] = (o, o.out)
            if "+backbone." in name:            # twin launch: the second conv's output is aux[3]
                last[int(name.split("+backbone.")[1].split(".")[0])] = (o, o.aux[3])
    base = plan.arena.data_ptr()
    checked = 0
    assert any("+backbone." in n for n in plan.op_names), "the side convs of the neck run as twin launches"
    for node, (o, out_ptr) in last.items():
        key = "tap64_%d" % node
        if key not in g.files:
            continue                            # heads are checked through featmaps above
        ref = g[key]
        Bn, Cn, Hn, Wn = ref.shape
        n_bytes = Bn * Hn * Wn * o.out_stride * 4
        off = out_ptr - base
        got = plan.arena[off:off + n_bytes].view(torch.float32).view(Bn, Hn, Wn, o.out_stride)[..., :Cn]
        np.testing.assert_allclose(got.permute(0, 3, 1, 2).cpu().numpy(), ref, rtol=1e-4, atol=5e-5, err_msg=key)
        checked += 1
    assert checked >= 20


def test_headline_shape_640_vs_reference_golden(golden, models):
    g = golden("maf_n")
    x = O.synth_images(2, 640, 1).to(DEV)
    with torch.no_grad():
        p32 = models["n"](x)[0]
        p16 = models["n"](x.half())[0]
    assert p32.shape == (2, 8400, 85)
    _close32(p32[:, ::16].cpu().numpy(), g["pred640_rows16"])
    np.testing.assert_allclose(p32.double().sum(1).cpu().numpy(), g["pred640_colsum"], rtol=1e-5, atol=1e-2)
    _close16(p16[:, ::16].cpu().numpy(), g["pred640_rows16"])
    dets, idx = M.non_max_suppression(p32, 0.03, 0.65, multi_label=True, return_index=True)
    odets, oidx = O.non_max_suppression(p32.cpu().numpy(), 0.03, 0.65, multi_label=True, return_index=True)
    for b in range(2):
        assert np.array_equal(dets[b].cpu().numpy(), odets[b]) and np.array_equal(idx[b].cpu().numpy(), oidx[b])


def test_config0_batch8_640_vs_reference_golden(golden, models):
    """BASELINE configs[0] at its stated batch — MAF-YOLO-n, 8 x 3 x 640 x 640, forward + NMS(0.03 / 0.65 / multi_label) as tools/eval.py runs them — against what the
    REFERENCE computed for the same eight images on the CPU (tests/golden/maf_n_b8.npz, tools/make_golden_b8.py): every 64th anchor row and the float64 column sums over
    all 8 400 anchors of the fp32 plan's prediction (north_star's 1e-3), the fp16 plan at its fp16-class bars, and the detections: the NMS of the fp32 prediction equals the
    oracle's on the same tensor bit for bit, and matches the reference's own rows (computed from ITS fp32 prediction, 1e-4 away) one to one where no pair sits at a threshold."""
    from nms_cases import match_detections
    g = golden("maf_n_b8")
    x = O.synth_images(8, 640, 1).to(DEV)
    with torch.no_grad():
        p32 = models["n"](x)[0]
        p16 = models["n"](x.half())[0]
    assert p32.shape == (8, 8400, 85)
    _close32(p32[:, ::64].cpu().numpy(), g["pred640_b8_rows64"])
    np.testing.assert_allclose(p32.double().sum(1).cpu().numpy(), g["pred640_b8_colsum"], rtol=1e-5, atol=1e-2)
    _close16(p16[:, ::64].cpu().numpy(), g["pred640_b8_rows64"])
    dets, idx = M.non_max_suppression(p32, 0.03, 0.65, multi_label=True, return_index=True)
    odets, oidx = O.non_max_suppression(p32.cpu().numpy(), 0.03, 0.65, multi_label=True, return_index=True)
    assert [d.shape[0] for d in dets] == list(g["nms640_b8_n"])
    for b in range(8):
        assert np.array_equal(dets[b].cpu().numpy(), odets[b]) and np.array_equal(idx[b].cpu().numpy(), oidx[b])
        ref = g["nms640_b8_%d" % b]
        pairs, miss, extra = match_detections(dets[b].cpu().numpy(), ref, iou_min=0.99, dscore=1e-3)
        assert len(pairs) >= ref.shape[0] - 3, (b, len(pairs), miss)     # (fp32 vs fp32: a row can only move at the max_det cut or at an IoU on the threshold)


def test_batch32_consistency_and_uint8_input(models):
    """BASELINE config[1] size: image i of a 32-batch gives the same rows as when run alone (fp16 engine);
    uint8 input with /255 folded into the stem equals float input."""
    m = models["n"]
    x = O.synth_images(32, 640, 9)
    with torch.no_grad():
        full = m(x.to(DEV).half())[0]
        one = m(x[5:6].to(DEV).half())[0]
    assert torch.equal(full[5:6], one)
    u8 = (x[:2] * 255).round().to(torch.uint8)
    with torch.no_grad():
        a = m(u8.to(DEV))[0]
        m.precision = "fp16"
        b = m((u8.float() / 255).to(DEV))[0]
        m.precision = None
    np.testing.assert_allclose(a.cpu().numpy()[..., 4:], b.cpu().numpy()[..., 4:], atol=2e-3)


def test_fresh_inputs_vs_oracle_all_scales(models):
    for s in "nsm":
        sd = O.synth_state_dict(s, 0)
        x = O.synth_images(2, 96, 21)
        ref = O.predict(O.reparam(sd, s), s, x).numpy()
        with torch.no_grad():
            p = models[s](x.to(DEV))[0].cpu().numpy()
        _close32(p, ref)


def test_state_dict_reload_invalidates_plans(models):
    m = M.Model("n").to(DEV).eval()
    x = O.synth_images(1, 64, 2).to(DEV)
    with torch.no_grad():
        a = m(x)[0].clone()
        m.load_state_dict(O.synth_state_dict("n", 0))
        b = m(x)[0]
    assert not torch.equal(a, b)
    assert torch.equal(b, models["n"](x)[0])


@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_nms_on_reference_predictions(golden, scale):
    g = golden("maf_" + scale)
    pred = torch.from_numpy(g["pred320_deploy"]).to(DEV)
    for tag, kw in (("eval", dict(conf_thres=0.03, iou_thres=0.65, multi_label=True)),
                    ("infer", dict(conf_thres=0.1, iou_thres=0.45, agnostic=True, max_det=1000)),
                    ("best", dict(conf_thres=0.05, iou_thres=0.45))):
        out = M.non_max_suppression(pred, **kw)
        assert isinstance(out, list) and out[0].device == pred.device and out[0].dtype == torch.float32
        assert np.array_equal(out[0].cpu().numpy(), g["nms320_%s" % tag]), (scale, tag)


@pytest.mark.parametrize("name", sorted(nms_cases.cases().keys()))
def test_nms_edge_cases_vs_reference_golden_and_oracle(golden, name):
    g = golden("nms_cases")
    pred, kw = nms_cases.cases()[name]
    out, idx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), return_index=True, **kw)
    oo, oi = O.non_max_suppression(pred, return_index=True, **kw)
    assert [o.shape[0] for o in out] == list(g[name + "__n"])
    for b, o in enumerate(out):
        assert o.shape[1] == 6
        assert np.array_equal(o.cpu().numpy(), g["%s__%d" % (name, b)]), (name, b)
        assert np.array_equal(idx[b].cpu().numpy(), oi[b]), (name, b)


@pytest.mark.parametrize("name", sorted(nms_cases.cases().keys()))
def test_nms_single_launch_form_is_bit_identical(golden, name, monkeypatch):
    """maf_nms_ex flag MAF_NMS_SINGLE_LAUNCH (csrc/nms.hip:nms_single_kernel — collect, then the last workgroup of every image sorts and selects:
    ONE launch for the whole of yolov6/utils/nms.py:31-105) against the same reference fixtures and oracle indices as the seven-launch form."""
    from maf_yolo_amd import nms as nms_mod
    monkeypatch.setattr(nms_mod, "SINGLE_LAUNCH_MAX_BATCH", 1 << 20)
    g = golden("nms_cases")
    pred, kw = nms_cases.cases()[name]
    out, idx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), return_index=True, **kw)
    _, oi = O.non_max_suppression(pred, return_index=True, **kw)
    assert [o.shape[0] for o in out] == list(g[name + "__n"])
    for b, o in enumerate(out):
        assert np.array_equal(o.cpu().numpy(), g["%s__%d" % (name, b)]), (name, b)
        assert np.array_equal(idx[b].cpu().numpy(), oi[b]), (name, b)


@pytest.mark.parametrize("matrix", [True, False])
@pytest.mark.parametrize("name", sorted(nms_cases.cases().keys()))
def test_nms_both_forms_of_the_all_pairs_path_are_bit_identical(golden, name, matrix, monkeypatch):
    """The two forms of the all-pairs path, each FORCED (nms.MATRIX_PATH; "auto" picks by situation: nms._matrix_form) — the n x n suppression bit matrix on the whole chip + a
    serial scan of its rows (maf_nms_ex flag MAF_NMS_MATRIX, rounds 2-5), and the kept-list scan (csrc/nms.hip:nms_greedy_kernel, round 6) — against the same reference
    fixtures and oracle indices."""
    from maf_yolo_amd import nms as nms_mod
    monkeypatch.setattr(nms_mod, "MATRIX_PATH", matrix)
    g = golden("nms_cases")
    pred, kw = nms_cases.cases()[name]
    out, idx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), return_index=True, **kw)
    _, oi = O.non_max_suppression(pred, return_index=True, **kw)
    assert [o.shape[0] for o in out] == list(g[name + "__n"])
    for b, o in enumerate(out):
        assert np.array_equal(o.cpu().numpy(), g["%s__%d" % (name, b)]), (name, b)
        assert np.array_equal(idx[b].cpu().numpy(), oi[b]), (name, b)


@pytest.mark.parametrize("max_det", [1, 64, 65, 300, 1000])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 700, 2500, 4096])
def test_nms_kept_list_scan_against_the_matrix_form_and_the_oracle(n_cand, max_det, monkeypatch):
    """The kept-list scan over every block boundary it has (one candidate, a ragged first block, exactly one / one-plus blocks, many blocks, the path's 4096-candidate
    limit) and kept-list lengths from 1 to past the block size and up to 1000: dense overlapping boxes in two classes (the benchmark's distribution: the all-pairs path),
    rows and indices equal to the oracle's and to the matrix form's."""
    from maf_yolo_amd import nms as nms_mod
    rng = np.random.RandomState(n_cand * 7 + max_det)
    N, nc = 8400, 80
    pred = np.zeros((2, N, 5 + nc), np.float32)
    for b in range(2):
        pred[b, :, 0:2] = rng.uniform(100, 540, (N, 2)); pred[b, :, 2:4] = rng.uniform(20, 160, (N, 2))
        pred[b, :, 4] = 1.0
        pred[b, :, 5:] = 0.001
        rows = rng.choice(N, n_cand, replace=False)
        pred[b, rows, 5 + 3 * rng.randint(0, 2, n_cand)] = rng.uniform(0.05, 0.99, n_cand).astype(np.float32)
    want, widx = O.non_max_suppression(pred, 0.03, 0.65, multi_label=True, max_det=max_det, return_index=True)
    x = torch.from_numpy(pred).to(DEV)
    monkeypatch.setattr(nms_mod, "MATRIX_PATH", False)
    got, gidx = M.non_max_suppression(x, 0.03, 0.65, multi_label=True, max_det=max_det, return_index=True)
    monkeypatch.setattr(nms_mod, "MATRIX_PATH", True)
    mat, midx = M.non_max_suppression(x, 0.03, 0.65, multi_label=True, max_det=max_det, return_index=True)
    for b in range(2):
        assert np.array_equal(gidx[b].cpu().numpy(), widx[b]) and np.array_equal(got[b].cpu().numpy(), want[b]), (n_cand, max_det, b)
        assert torch.equal(gidx[b], midx[b]) and torch.equal(got[b], mat[b]), (n_cand, max_det, b)


@pytest.mark.parametrize("conf,kw", [(0.03, dict(iou_thres=0.65, multi_label=True)), (0.25, dict(iou_thres=0.45, multi_label=True, agnostic=True)),
                                     (0.001, dict(iou_thres=0.65, multi_label=True, max_det=1000))])
def test_candidate_filter_inside_the_forward_gives_the_same_detections(models, conf, kw):
    """Model.nms_filter = conf_thres: the head tails append the candidates of the NMS call that follows to its workspace (maf_engine_run_filtered,
    MAF_NMS_PRECOLLECTED — yolov6/utils/nms.py:48,69,75-77 folded into the kernels that compute the scores): rows and flat indices bit-identical to
    the two-step path, for several thresholds, twice in a row on the same slot (workspace reuse), and a call that filters differently (other conf,
    best-class mode) falls back to its own pass over the prediction."""
    m = models["n"]
    x = O.synth_images(2, 640, 5).to(DEV).half()
    ref_pred = m(x)[0]
    want, widx = M.non_max_suppression(ref_pred, conf, return_index=True, **kw)
    m.nms_filter = conf
    try:
        small = m(O.synth_images(1, 320, 5).to(DEV).half())[0]              # 10 x 10 level: not a multiple of 16 pixels -> the plain forward
        assert getattr(small, "_maf_cand", None) is None
        for _ in range(2):
            pred = m(x)[0]
            assert getattr(pred, "_maf_cand", None) is not None and torch.equal(pred, ref_pred)
            got, gidx = M.non_max_suppression(pred, conf, return_index=True, **kw)
            assert pred._maf_cand is None                                    # consumed
            for a_, b_, ia, ib in zip(got, want, gidx, widx):
                assert torch.equal(a_, b_) and torch.equal(ia, ib)
        pred = m(x)[0]
        other = M.non_max_suppression(pred, conf * 2, iou_thres=0.5)         # different filter: the lists are not used
        assert pred._maf_cand is not None
        base = M.non_max_suppression(ref_pred, conf * 2, iou_thres=0.5)
        for a_, b_ in zip(other, base):
            assert torch.equal(a_, b_)
        h = M.non_max_suppression_async(m(x)[0], conf, **kw)                 # the serving loop's form, NMS on a side stream
        for a_, b_ in zip(h.result(), want):
            assert torch.equal(a_, b_)
        # the lists belong to ONE forward: a second forward into the slot before the first prediction's NMS refills them, and the NMS of the
        # first prediction must not read forward 2's lists (advisor finding, round 3) — it falls back to its own pass
        x2 = O.synth_images(2, 640, 6).to(DEV).half()
        p1 = m(x)[0]
        p2 = m(x2)[0]
        got1 = M.non_max_suppression(p1, conf, **kw)
        assert p1._maf_cand is not None                                      # stale generation: not used, not consumed
        for a_, b_ in zip(got1, want):
            assert torch.equal(a_, b_)
        want2 = M.non_max_suppression(p2.clone(), conf, **kw)
        got2 = M.non_max_suppression(p2, conf, **kw)
        assert p2._maf_cand is None
        for a_, b_ in zip(got2, want2):
            assert torch.equal(a_, b_)
        # ... and to the tensor AS WRITTEN: an in-place edit of the prediction invalidates them
        p3 = m(x)[0]
        p3[..., 5:] *= 0.5
        got3 = M.non_max_suppression(p3, conf, **kw)
        want3 = M.non_max_suppression(p3.clone(), conf, **kw)
        for a_, b_ in zip(got3, want3):
            assert torch.equal(a_, b_)
    finally:
        m.nms_filter = None


def test_nms_large_candidate_set_global_sort_path():
    """> 8192 candidates per image: sort runs in global memory; > 30000: top-30000 rule."""
    rs = np.random.RandomState(3)
    n, nc = 2000, 80
    b = np.concatenate([rs.rand(n, 2) * 600, 5 + rs.rand(n, 2) * 60], 1).astype(np.float32)
    cls = (rs.rand(n, nc) ** 3).astype(np.float32)
    pred = np.concatenate([b, np.ones((n, 1), np.float32), cls], 1)[None]
    for conf in (0.5, 0.2, 0.001):
        out, idx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), conf, 0.6, multi_label=True, return_index=True)
        oo, oi = O.non_max_suppression(pred, conf, 0.6, multi_label=True, return_index=True)
        assert np.array_equal(out[0].cpu().numpy(), oo[0]) and np.array_equal(idx[0].cpu().numpy(), oi[0]), conf


def test_nms_fp16_prediction_is_upcast():
    pred, kw = nms_cases.cases()["clustered_eval"]
    h = torch.from_numpy(pred).half()
    out = M.non_max_suppression(h.to(DEV), **kw)
    oo = O.non_max_suppression(h.float().numpy(), **kw)
    for a, b in zip(out, oo):
        assert np.array_equal(a.cpu().numpy(), b)


def test_async_nms_matches_sync(models):
    x = O.synth_images(2, 320, 5).to(DEV)
    with torch.no_grad():
        pred = models["n"](x)[0]
    ref = M.non_max_suppression(pred, 0.03, 0.65, multi_label=True)
    hs = [M.non_max_suppression_async(pred, 0.03, 0.65, multi_label=True) for _ in range(4)]     # several in flight
    for h in hs:
        out = h.result()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


@pytest.mark.parametrize("thr", [0.0, 0.1, 1.0 / 3.0, 0.45, 0.5, 0.65, 0.75, 0.9, 1.0])
def test_nms_division_free_iou_is_exact(thr):
    """Heavily overlapping same-class boxes on an integer grid: many IoUs are simple rationals that hit the threshold
    exactly (1/3, 1/2, 3/4 ...), which is where a rounding shortcut would show."""
    rs = np.random.RandomState(int(thr * 1000) + 1)
    n, nc = 400, 3
    xy = rs.randint(0, 12, (n, 2)).astype(np.float32) * 4
    wh = rs.randint(1, 7, (n, 2)).astype(np.float32) * 8
    b = np.concatenate([xy + wh / 2 + 100, wh], 1).astype(np.float32)
    cls = (0.2 + 0.8 * rs.rand(n, nc)).astype(np.float32)
    pred = np.concatenate([b, np.ones((n, 1), np.float32), cls], 1)[None]
    out, idx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), 0.25, thr, multi_label=True, max_det=1000, return_index=True)
    oo, oi = O.non_max_suppression(pred, 0.25, thr, multi_label=True, max_det=1000, return_index=True)
    assert np.array_equal(idx[0].cpu().numpy(), oi[0]) and np.array_equal(out[0].cpu().numpy(), oo[0])


def test_hipgraph_replay_equals_eager(models):
    """bs=1 latency path (BASELINE configs[4]): the plan replayed from a captured hipGraph gives the same bits."""
    m = models["m"]
    x = O.synth_images(1, 320, 3).to(DEV).half()
    with torch.no_grad():
        eager = m(x)[0].clone()
        plan = m.plan_for(x)
        pred = torch.empty_like(eager)
        for _ in range(3):                          # capture on first call, replay afterwards
            plan.run_into(x, pred, graph=True)
        torch.cuda.synchronize()
    assert torch.equal(pred, eager)
    x2 = O.synth_images(1, 320, 4).to(DEV).half()   # new data in the SAME input buffer is picked up by the replay
    x.copy_(x2)
    with torch.no_grad():
        plan.run_into(x, pred, graph=True)
        ref = m(x2)[0]
    torch.cuda.synchronize()
    assert torch.equal(pred, ref)


def test_autotuned_tiles_give_identical_predictions(models):
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0))
    m = m.to(DEV).eval()
    x = O.synth_images(4, 320, 6).to(DEV).half()
    with torch.no_grad():
        base = m(x)[0].clone()
        plan = m.plan_for(x)
        plan.autotune(x)
        tuned = m(x)[0]
    # a tile only re-cuts the (pixel, channel) space; only the split-K variants change a summation order (fp32 partials)
    _close16(tuned.cpu().numpy(), base.cpu().numpy())


def test_fused_bottleneck_plan_matches_unfused(models):
    """MAF_OP_BOTTLENECK / MAF_OP_CONV1DW plans (full fusion for c <= 64, conv1+dw elsewhere; conv1+dw everywhere) vs three kernels."""
    outs = {}
    for fuse in (True, 2, False):
        m = M.Model("n")
        m.load_state_dict(O.synth_state_dict("n", 0))
        m = m.to(DEV).eval()
        m.fuse_bottlenecks = fuse
        x = O.synth_images(2, 320, 8).to(DEV).half()
        with torch.no_grad():
            outs[fuse] = m(x)[0].cpu().numpy()
        assert sum(1 for o in m.plan_for(x).ops if o.kind == 6) == (6 if fuse is True else 0)
        assert sum(1 for o in m.plan_for(x).ops if o.kind == 7) == {True: 4, 2: 10, False: 0}[fuse]
    _close16(outs[True], outs[False])
    _close16(outs[2], outs[False])


@pytest.mark.parametrize("scale,shape,ntail", [("n", (2, 320, 320), 4), ("n", (3, 352, 288), 4), ("s", (2, 320, 256), 2), ("m", (2, 256, 256), 1)])
def test_closing_conv_inside_the_bottleneck_launch_matches_the_two_launches(scale, shape, ntail):
    """MAF_OP_BOTTLENECK with op.nc (the RepHDW block's conv2(cat(..)) + SiLU applied inside the launch of its last bottleneck, csrc/bottleneck.hip) against the
    same plan with the closing conv as its own launch: same fp16 rounding points (the bottleneck's output is rounded to fp16 before the closing GEMM either
    way), another fp32 summation order.  n takes it by default (one bottleneck per block), s / m on request (two: their second bottleneck carries the conv)."""
    B, H, W = shape
    x = O.synth_images(B, max(H, W), 5)[:, :, :H, :W].contiguous().to(DEV).half()
    outs = {}
    for ft in (True, False):
        m = M.Model(scale)
        m.load_state_dict(O.synth_state_dict(scale, 0))
        m = m.to(DEV).eval()
        m.fuse_tail = ft
        with torch.no_grad():
            outs[ft] = m(x)[0].float().cpu().numpy()
        plan = m.plan_for(x)
        assert sum(1 for o in plan.ops if o.kind == 6 and o.nc) == (ntail if ft else 0)
        for n_ in plan.op_names:                               # a block whose bottleneck carries the conv has no conv2 launch of its own
            if n_.endswith("+conv2"):
                assert n_.split(".m.")[0] + ".conv2" not in plan.op_names
    _close16(outs[True], outs[False], scale)


@pytest.mark.parametrize("shape,scale", [((2, 320, 320), "n"), ((3, 256, 384), "n"), ((32, 640, 640), "n"), ((2, 320, 256), "s")])
def test_fused_head_tail_matches_unfused(shape, scale):
    """MAF_OP_HEADTAIL ({cls,reg}_conv_s -> pred -> sigmoid / DFL decode, one launch per level) vs four 1x1 convs + the decode kernel:
    same fp16 rounding points, so only the fp32 summation order differs."""
    B, H, W = shape
    x = O.synth_images(B, max(H, W), 21)[:, :, :H, :W].contiguous().to(DEV).half()
    outs = {}
    nlev = {"n": 3, "s": 3}[scale]                      # s: the 256-wide P5 level streams its weights through LDS in chunks (small levels only)
    for fh in (True, False):
        m = M.Model(scale)
        m.load_state_dict(O.synth_state_dict(scale, 0))
        m = m.to(DEV).eval()
        m.fuse_head = fh
        with torch.no_grad():
            pred, feats = m(x)
        outs[fh] = pred.float().cpu().numpy()
        kinds = [o.kind for o in m.plan_for(x).ops]
        assert (kinds.count(8) == nlev and kinds.count(5) == (nlev < 3)) if fh else (8 not in kinds and kinds.count(5) == 1)
        assert (feats[0][1] is None) == fh and feats[0][0] is not None
        if fh:                                    # asking for the head tensors (val_loss) selects a plan that materialises them
            with torch.no_grad():
                _, feats2 = m(x, val_loss=True)
            assert feats2[2][1].shape == (B, 80, H // 32, W // 32) and feats2[2][2].shape == (B, 68, H // 32, W // 32)
    a, b = outs[True], outs[False]
    assert np.array_equal(a[..., 4], b[..., 4]) and np.all(a[..., 4] == 1.0)
    assert np.abs(a[..., 5:] - b[..., 5:]).max() <= 3e-3
    assert np.abs(a[..., :4] - b[..., :4]).max() <= 0.05 + 2e-3 * np.abs(b[..., :4]).max()
    assert np.abs(a[..., :4] - b[..., :4]).mean() <= 2e-3


@pytest.mark.parametrize("shape,dt,scale", [((2, 320, 320), "f16", "n"), ((3, 256, 384), "u8", "n"), ((2, 352, 608), "f16", "n"), ((32, 640, 640), "u8", "n"),
                                            ((1, 64, 96), "f32", "n"), ((2, 320, 352), "f16", "s"), ((2, 96, 64), "u8", "s"),
                                            ((2, 320, 288), "f16", "m"), ((1, 96, 160), "u8", "m")])
def test_fused_stem_matches_unfused(shape, dt, scale):
    """MAF_OP_STEM2 (backbone.0 + backbone.1 in one launch, both on the matrix cores, the half-resolution tensor in LDS) vs the VALU stem +
    the 3x3 s2 MFMA conv: node 1's output to fp16 rounding (the fused stem rounds its weights to fp16, the VALU stem keeps them fp32),
    predictions within the fp16 class.  Tiles that hang over the map (88 x 152, 16 x 24) and every input dtype."""
    B, H, W = shape
    img = O.synth_images(B, max(H, W), 23)[:, :, :H, :W].contiguous()
    x = {"f16": img.half(), "f32": img, "u8": (img * 255).round().to(torch.uint8)}[dt].to(DEV)
    outs, taps, nops = {}, {}, {}
    for fs in (2, 1, 0):                           # 2 (= True): stem pair + the 1x1 that opens backbone.2; 1: stem pair; 0: three launches
        m = M.Model(scale, precision="fp16")
        m.load_state_dict(O.synth_state_dict(scale, 0))
        m = m.to(DEV).eval()
        m.fuse_stem = fs
        with torch.no_grad():
            outs[fs] = m(x)[0].float().cpu().numpy()
        plan = m.plan_for(x)
        assert (plan.ops[0].kind == 9) == bool(fs) and plan.ops[0].nc == (plan.ops[0].Cout if fs == 2 else 0)
        nops[fs] = len(plan.ops)
        # the tensor all three modes materialise: the output of backbone.2.conv1 = the first channels of node 2's concat buffer
        o = plan.ops[[i for i, nme in enumerate(plan.op_names) if nme.endswith("2.conv1")][0]]
        c3 = o.nc if o.kind == 9 else o.Cout
        def rd(ptr, stride, c):
            off = ptr - plan.arena.data_ptr()
            return plan.arena[off:off + B * (H // 4) * (W // 4) * stride * 2].view(torch.float16).view(B, H // 4, W // 4, stride)[..., :c].float().cpu()
        if o.kind == 9 and o.aux[0]:               # the fused stem hands the two halves (RepHDW's chunk(2)) to two dense tensors
            taps[fs] = torch.cat([rd(o.out, o.out_stride, c3 // 2), rd(o.aux[0], o.reg_stride, c3 // 2)], -1).numpy()
        else:
            taps[fs] = rd(o.out, o.out_stride, c3).numpy()
    assert nops[2] == nops[0] - 2 and nops[1] == nops[0] - 1
    # the 4-row tile variant (tile_p = 4: what the autotuner may pick) computes every output pixel with the same operations: bitwise equal
    m.fuse_stem = True
    plan8 = m.plan_for(x)
    o8 = plan8.ops[0]
    assert o8.kind == 9
    spans = [(o8.out - plan8.arena.data_ptr(), B * (H // 4) * (W // 4) * o8.out_stride * 2)]
    if o8.aux[0]:
        spans.append((o8.aux[0] - plan8.arena.data_ptr(), B * (H // 4) * (W // 4) * o8.reg_stride * 2))
    res = []
    for rows, wgs in ((8, 0), (4, 300)):
        o8.tile_p, o8.tile_k = rows, wgs
        for off, nbytes in spans:
            plan8.arena[off:off + nbytes].zero_()
        plan8.launch_op(0, image_ptr=x.contiguous().data_ptr())
        torch.cuda.synchronize()
        res.append(torch.cat([plan8.arena[off:off + nbytes] for off, nbytes in spans]))
    o8.tile_p, o8.tile_k = 0, 0
    assert torch.equal(res[0], res[1]) and res[0].any()
    for fs in (2, 1):
        d = np.abs(taps[fs] - taps[0])
        assert d.max() <= 2e-2 * max(1.0, np.abs(taps[0]).max()) and d.mean() <= 1e-3 * max(1.0, np.abs(taps[0]).mean()), fs
        _close16(outs[fs], outs[0], scale)


def test_tuned_plan_at_the_benchmark_size_matches_the_default_plan(models):
    """BASELINE configs[1] as bench.py runs it — 32 x 640^2, fp16, autotune on: the tuned plan carries what only tuned plans have (MPRep of backbone.3 as ONE
    launch of the LDS-resident 3x3 kernel, csrc/conv3s2_lds.hip with nc) beside the dense concat slots behind the fused stem, and its predictions equal the
    untuned default plan's (one launch list for every batch size, generic tiles) within the fp16 class; image i of the batch equals image i run alone."""
    x = O.synth_images(32, 640, 17).to(DEV).half()
    with torch.no_grad():
        ref = models["n"](x)[0].float().cpu().numpy()
        one = models["n"](x[7:8])[0].float().cpu().numpy()
    from maf_yolo_amd import lib
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0))
    m = m.to(DEV).eval()
    m.autotune = True
    with torch.no_grad():
        got = m(x)[0].float().cpu().numpy()
    plan = m.plan_for(x)
    fused = [o for o, n_ in zip(plan.ops, plan.op_names) if n_ == "backbone.3.conv1+conv2"]
    assert len(fused) == 1 and (fused[0].kind, fused[0].tile_k, fused[0].nc, fused[0].reg_stride, fused[0].out_coff) == (lib.OP_CONV3X3S2, 6, 48, 0, 48)
    tail = plan.ops[plan.op_names.index("backbone.2.m.0+conv2")]              # backbone.2's closing conv rides in its bottleneck's launch: the two dense slots are its sources
    assert plan.ops[0].kind == lib.OP_STEM2 and plan.ops[0].aux[0] and tail.kind == lib.OP_BOTTLENECK and tail.nsrc == 2 and tail.nc == 48 and tail.src[0].ptr != tail.src[1].ptr
    assert len(plan.ops) == len(models["n"].plan_for(x).ops) - 1
    assert np.isfinite(got).all()
    _close16(got, ref, "n")
    _close16(got[7:8], one, "n")


def test_fusion_choice_is_measured_when_autotuning():
    from maf_yolo_amd import engine
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0))
    m = m.to(DEV).eval()
    m.autotune = True
    x = O.synth_images(2, 320, 8).to(DEV).half()
    with torch.no_grad():
        m(x)
    plan = m.plan_for(x)
    decided = [k for k in engine._TUNE_CACHE if k[0] == "bn3" and k[2] == 2 and k[3] in (80, 40, 20, 10)]
    assert len(decided) >= 4                       # one decision per distinct bottleneck signature
    nf, npart = sum(1 for o in plan.ops if o.kind == 6), sum(1 for o in plan.ops if o.kind == 7)
    ntail = sum(1 for o in plan.ops if o.kind == 6 and o.nc)          # fully fused bottlenecks that also carry their block's closing conv
    assert len(plan.ops) == 73 - 2 * nf - npart - ntail   # 90 launches unfused; fused head (one depth-wise + one tail per level): -13; fused stem + backbone.2.conv1: -2; twin side convs: -2


def test_post_nms_tail_matches_reference_fixture(golden):
    """f4: convert_to_coco_format on the device == the reference's Evaler.convert_to_coco_format (tools/make_golden_post.py)."""
    g = golden("post_cases")
    ids = g["ids"].tolist()
    for ci in range(3):
        counts = g["c%d_counts" % ci]
        dets = torch.from_numpy(g["c%d_dets" % ci])
        outs, o = [], 0
        for n in counts:
            outs.append(dets[o:o + int(n)].to(DEV)); o += int(n)
        shapes = [((s[0], s[1]), ((s[2], s[3]), (s[4], s[5]))) for s in g["c%d_shapes" % ci]]
        paths = ["/x/%012d.jpg" % i for i in g["c%d_image_ids" % ci]]
        res = M.convert_to_coco_format(outs, torch.zeros(len(outs), 3, 640, 640), paths, shapes, ids, is_coco=True,
                                       scale_exact=bool(g["c%d_scale_exact" % ci]))
        assert [r["image_id"] for r in res] == g["c%d_out_image_id" % ci].tolist()
        assert [r["category_id"] for r in res] == g["c%d_out_category_id" % ci].tolist()
        assert np.array_equal(np.asarray([r["bbox"] for r in res]).reshape(-1, 4), g["c%d_out_bbox" % ci])
        assert np.array_equal(np.asarray([r["score"] for r in res]), g["c%d_out_score" % ci])


def test_post_nms_tail_from_device_nms_result(models):
    """The tail consumes the NMS result without a host round trip; equals the oracle on the same detections."""
    x = O.synth_images(3, 320, 5).to(DEV)
    with torch.no_grad():
        pred = models["n"](x)[0]
    raw = M.nms_raw(pred, 0.03, 0.65, multi_label=True)
    shapes = [((480, 640), ((0.5, 0.5), (0.0, 40.0))), ((333, 500), ((0.64, 0.64), (0.0, 53.44))), ((1080, 1920), ((1 / 6, 1 / 6), (0.0, 70.0)))]
    ids = list(range(1, 81))
    res = M.convert_to_coco_format(raw, x, ["1.jpg", "2.jpg", "3.jpg"], shapes, ids)
    counts = raw[2].tolist()
    outs = [raw[0][b, :n].cpu().numpy() for b, n in enumerate(counts)]
    iid, cid, bb, sc = O.coco_rows(outs, shapes, [1, 2, 3], ids)
    assert len(res) == sum(counts) and [r["image_id"] for r in res] == iid.tolist() and [r["category_id"] for r in res] == cid.tolist()
    assert np.array_equal(np.asarray([r["bbox"] for r in res]).reshape(-1, 4), bb) and np.array_equal(np.asarray([r["score"] for r in res]), sc)


def test_checkpoint_bridge_forward_matches_reference_output(golden):
    """f3: weights read from a reference-pickled checkpoint drive the HIP engine to the reference model's own prediction."""
    import os
    from maf_yolo_amd import checkpoint
    g = golden("ref_ckpt_tiny")
    m = checkpoint.load_checkpoint(os.path.join(os.path.dirname(__file__), "golden", "ref_ckpt_tiny.pt")).to(DEV)
    x = O.synth_images(1, 64, 3).to(DEV)
    with torch.no_grad():
        pred = m(x)[0].cpu().numpy()
    ref = g["pred"]
    assert pred.shape == ref.shape
    assert np.abs(pred[..., :4] - ref[..., :4]).max() <= 1e-3 + 1e-5 * np.abs(ref[..., :4]).max()
    assert np.abs(pred[..., 4:] - ref[..., 4:]).max() <= 2e-5


def test_multi_stream_plan_equals_single_stream(models):
    """Lanes only change WHEN an op runs: outputs are bitwise those of the single-stream plan, eager and from the hipGraph."""
    x = O.synth_images(4, 320, 11).to(DEV).half()
    outs = {}
    for ms in (2, 1, False):
        m = M.Model("n")
        m.load_state_dict(O.synth_state_dict("n", 0))
        m = m.to(DEV).eval()
        m.multi_stream = ms
        m.fuse_head = False                      # the fused head tail is a single-stream variant: compare like with like
        with torch.no_grad():
            outs[ms] = m(x)[0].clone()
            plan = m.plan_for(x)
            assert (max(o.lane for o in plan.ops) > 0) == bool(ms)
            pred = torch.empty_like(outs[ms])
            for _ in range(3):
                plan.run_into(x, pred, graph=True)
            torch.cuda.synchronize()
            assert torch.equal(pred, outs[ms])
    assert torch.equal(outs[2], outs[False]) and torch.equal(outs[1], outs[False])


@pytest.mark.parametrize("hw", [(384, 640), (352, 608), (64, 96)])
def test_rectangular_images_vs_oracle(models, hw):
    """Rect inference (evaler.py pads to multiples of 32, not to squares): every level's grid is H/s x W/s."""
    g = torch.Generator().manual_seed(hw[0] + hw[1])
    x = torch.rand(2, 3, hw[0], hw[1], generator=g)
    sd = {k: v.detach().cpu() for k, v in models["n"].state_dict().items()}
    ref = O.predict(O.reparam(sd, "n"), "n", x).numpy()
    with torch.no_grad():
        got = models["n"](x.to(DEV))[0].cpu().numpy()
    assert got.shape == ref.shape == (2, (hw[0] // 8) * (hw[1] // 8) + (hw[0] // 16) * (hw[1] // 16) + (hw[0] // 32) * (hw[1] // 32), 85)
    _close32(got, ref)
    with torch.no_grad():
        got16 = models["n"](x.to(DEV).half())[0].cpu().numpy()
    _close16(got16, ref)


@pytest.mark.parametrize("n_cand", [4095, 4096, 4097, 6000])
def test_nms_matrix_and_list_paths_meet_at_4096_candidates(n_cand):
    """<= 4096 candidates: suppression-matrix kernels; more: the one-workgroup greedy kernel (LDS sort up to 8192).  Same answer."""
    rng = np.random.RandomState(n_cand)
    N, nc = 9000, 6
    pred = np.zeros((1, N, 5 + nc), np.float32)
    pred[0, :, 0:2] = rng.uniform(40, 600, (N, 2)); pred[0, :, 2:4] = rng.uniform(8, 90, (N, 2))
    pred[0, :, 4] = 1.0
    pred[0, :, 5:] = 0.01
    rows = rng.choice(N, n_cand, replace=False)
    pred[0, rows, 5 + rng.randint(0, nc, n_cand)] = rng.uniform(0.3, 0.99, n_cand).astype(np.float32)     # exactly n_cand candidates > conf
    want, widx = O.non_max_suppression(pred, 0.25, 0.5, multi_label=True, max_det=300, return_index=True)
    got, gidx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), 0.25, 0.5, multi_label=True, max_det=300, return_index=True)
    assert np.array_equal(gidx[0].cpu().numpy(), widx[0]) and np.array_equal(got[0].cpu().numpy(), want[0])


@pytest.mark.parametrize("case", ["balanced", "dominant_class", "huge_boxes", "agnostic", "ties"])
def test_nms_per_class_path_and_matrix_path_agree_with_oracle(case):
    """nms_sort_kernel sends an image down the per-class path (class-major sort, one short scan per class, survivors re-sorted by score)
    when no class holds more than 256 candidates and no box can reach another class's 4096-px band, else down the all-pairs matrix path.
    Both must give the oracle's rows and indices bit for bit: balanced classes (per-class), one class with ~1500 candidates (matrix),
    boxes wider than a band (matrix), class-agnostic (matrix), and many equal scores in the per-class path (tie order = flat index)."""
    rng = np.random.RandomState(7)
    N, nc, n_cand = 8400, 80, 2200
    pred = np.zeros((2, N, 5 + nc), np.float32)
    for b in range(2):
        pred[b, :, 0:2] = rng.uniform(30, 610, (N, 2)); pred[b, :, 2:4] = rng.uniform(10, 120, (N, 2))
        pred[b, :, 4] = 1.0
        pred[b, :, 5:] = 0.001
        rows = rng.choice(N, n_cand, replace=True)
        cls = rng.randint(0, nc, n_cand)
        if case == "dominant_class":
            cls[: 1500] = 17
        sc = rng.uniform(0.05, 0.99, n_cand).astype(np.float32)
        if case == "ties":
            sc = (np.round(sc * 20) / 20).astype(np.float32)
        pred[b, rows, 5 + cls] = sc
        if case == "huge_boxes":
            pred[b, rows[:5], 2:4] = 5000.0
    kw = dict(multi_label=True, max_det=300, agnostic=(case == "agnostic"))
    want, widx = O.non_max_suppression(pred, 0.03, 0.65, return_index=True, **kw)
    got, gidx = M.non_max_suppression(torch.from_numpy(pred).to(DEV), 0.03, 0.65, return_index=True, **kw)
    for b in range(2):
        assert np.array_equal(gidx[b].cpu().numpy(), widx[b]), (case, b)
        assert np.array_equal(got[b].cpu().numpy(), want[b]), (case, b)


def test_two_batches_in_flight_on_two_streams_give_the_single_stream_result(models):
    """Model.forward(slot=k): plans of different slots own different arenas, so consecutive batches may run concurrently on different HIP
    streams (bench.py's serving loop).  Interleaved on two streams, with the NMS on the side stream, every batch gives bitwise the
    predictions and detections of a lone forward."""
    m = models["n"]
    xs = [O.synth_images(4, 320, 30 + i).to(DEV).half() for i in range(4)]
    with torch.no_grad():
        want = [m(x)[0].clone() for x in xs]
    wdets = [M.non_max_suppression(p, 0.03, 0.65, multi_label=True) for p in want]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV) for _ in range(2)]
    for rep in range(3):
        preds, handles = [], []
        for i, x in enumerate(xs):
            with torch.cuda.stream(streams[i % 2]), torch.no_grad():
                p = m(x, slot=i % 2)[0]
                preds.append(p)
                handles.append(M.non_max_suppression_async(p, 0.03, 0.65, multi_label=True))
        dets = [h.result() for h in handles]
        torch.cuda.synchronize()
        for i in range(4):
            assert torch.equal(preds[i], want[i]), (rep, i)
            assert all(torch.equal(a, b) for a, b in zip(dets[i], wdets[i])), (rep, i)
    assert m.plan_for(xs[0], slot=0) is not m.plan_for(xs[0], slot=1)
    assert m.plan_for(xs[0], slot=0).arena.data_ptr() != m.plan_for(xs[0], slot=1).arena.data_ptr()


def test_concurrent_streams_overlap():
    """streams.concurrent_streams: the streams it returns run spin kernels side by side (streams that alias onto one hardware queue —
    which plain torch.cuda.Stream() pairs sometimes do — would take n times as long).  Three streams, or as many as the hardware queues the
    environment grants a process, if that is fewer: beyond that even distinct queues cannot be had."""
    import os
    import time
    cap = os.environ.get("GPU_MAX_HW_QUEUES")
    n = 3 if cap is None else max(2, min(3, int(cap)))
    ss = M.concurrent_streams(DEV, n)
    assert len({s.cuda_stream for s in ss}) == n
    def spin(streams):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in streams:
            with torch.cuda.stream(s):
                torch.cuda._sleep(4_000_000)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    spin(ss[:1])
    one = min(spin(ss[:1]) for _ in range(3))
    together = min(spin(ss) for _ in range(3))
    assert together < (n + 1) / 2 * one, (n, one, together)           # two streams on one queue: n = 3 -> 2x, n = 2 -> 2x


def test_async_nms_of_fp16_and_strided_predictions_is_ordered_after_their_producer(models):
    """the fp16 -> fp32 cast / compaction of the prediction must run on the side stream (after its wait on the producer), not
    on the current stream after the wait was issued.  The producer is delayed with a spin kernel so that a mis-ordered read would see
    the buffer before the values are there."""
    x = O.synth_images(2, 320, 5).to(DEV)
    with torch.no_grad():
        pred = models["n"](x)[0]
    want = M.non_max_suppression(pred.half().float(), 0.03, 0.65, multi_label=True)
    wide = torch.zeros(2, pred.shape[1], 96, device=DEV)
    for rep in range(3):
        buf16 = torch.zeros_like(pred, dtype=torch.float16)
        torch.cuda._sleep(20_000_000)                        # ~10 ms: everything below is queued behind it on the current stream
        buf16.copy_(pred)
        wide.zero_(); wide[..., 3:88].copy_(pred.half().float())
        h1 = M.non_max_suppression_async(buf16, 0.03, 0.65, multi_label=True)
        h2 = M.non_max_suppression_async(wide[..., 3:88], 0.03, 0.65, multi_label=True)
        for h in (h1, h2):
            out = h.result()
            assert all(torch.equal(a, b) for a, b in zip(out, want)), rep


def test_eval_plans_follow_in_place_weight_updates(models):
    """an eval-mode model whose weights are updated in place (the reference's EMA model, engine.py:246) must not keep running
    the weights packed at its first forward."""
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0))
    m = m.to(DEV).eval()
    x = O.synth_images(1, 64, 2).to(DEV)
    with torch.no_grad():
        a = m(x)[0].clone()
        assert torch.equal(m(x)[0], a) and len(m._plans) == 1
        sd2 = O.synth_state_dict("n", 1)
        for (k, p) in m.state_dict().items():                # EMA-style in-place update, no train() / load_state_dict() call
            p.mul_(0.5).add_(0.5 * sd2[k].to(p.device, p.dtype)) if p.dtype.is_floating_point else None
        b = m(x)[0].clone()
    assert not torch.equal(a, b)
    ref = M.Model("n")
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(ref.to(DEV).eval()(x)[0], b)


@pytest.mark.parametrize("nc", [1, 3, 7, 81])
def test_any_class_count_runs_and_matches_the_sliced_80_class_model(models, nc):
    """the reference takes any `nc`; the conv kernels store 4 channels at a time, so cls_pred is padded internally.  A model
    with nc classes whose cls_pred filters are the first nc (or, for 81, the 80 + one extra) of the 80-class model must reproduce the
    corresponding prediction columns; fp32 plan vs the oracle's 80-class prediction, fp16 plan within the fp16 class."""
    sd = O.synth_state_dict("n", 0)
    sd_nc = dict(sd)
    for k in list(sd):
        if k.endswith("cls_pred.weight") or k.endswith("cls_pred.bias"):
            v = sd[k]
            sd_nc[k] = v[:nc].clone() if nc <= 80 else torch.cat([v, v[:nc - 80]], 0)
    m = M.Model("n", num_classes=nc)
    m.load_state_dict(sd_nc)
    m = m.to(DEV).eval()
    x = O.synth_images(2, 96, 21)
    ref = O.predict(O.reparam(sd, "n"), "n", x).numpy()
    cols = list(range(5 + min(nc, 80))) + ([5 + i for i in range(nc - 80)] if nc > 80 else [])
    with torch.no_grad():
        p32, feats = m(x.to(DEV), val_loss=False)
        p16 = m(x.to(DEV).half())[0]
        (f_, cls_t, reg_t), _ = m(x.to(DEV), val_loss=True)
    assert p32.shape == (2, 144 + 36 + 9, 5 + nc) and cls_t.shape == (2, 189, nc) and feats[0][1].shape == (2, nc, 12, 12)
    _close32(p32.cpu().numpy(), ref[..., cols])
    _close16(p16.cpu().numpy(), ref[..., cols])
    dets = M.non_max_suppression(p32, 0.03, 0.65, multi_label=True)
    odets = O.non_max_suppression(p32.cpu().numpy(), 0.03, 0.65, multi_label=True)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(dets, odets))


@pytest.mark.parametrize("half", [True, False])
def test_twin_conv_launch_equals_two_launches(models, half):
    """backbone.23 / .24 and .27 / .28 (equal, independent ConvWrappers) as ONE launch each (blockIdx.y picks the conv): the same
    instructions on the same data as two launches -> bitwise equal predictions, two ops fewer; also after autotuning."""
    x = O.synth_images(3, 320, 12).to(DEV)
    x = x.half() if half else x
    outs = {}
    for tw in (True, False):
        m = M.Model("n")
        m.load_state_dict(O.synth_state_dict("n", 0))
        m = m.to(DEV).eval()
        m.twin_convs = tw
        with torch.no_grad():
            outs[tw] = m(x)[0].clone()
        names = m.plan_for(x).op_names
        assert sum("+backbone." in n for n in names) == (2 if tw else 0)
        outs[tw, "n"] = len(names)
        if tw and half:
            plan = m.plan_for(x)
            plan.autotune(x)
            with torch.no_grad():
                tuned = m(x)[0]
            _close16(tuned.cpu().numpy(), outs[tw].cpu().numpy())
    assert outs[True, "n"] == outs[False, "n"] - 2
    assert torch.equal(outs[True], outs[False])


@pytest.mark.parametrize("fold", [True, False])
def test_eval_loop_matches_the_reference_evaler_fixture(golden, fold):
    """SURVEY.md 8(c) / VERDICT r1 missing #4: EvalLoop.predict_model — uint8 batch -> /255 -> model(imgs)[0] -> NMS(0.03, 0.65, multi_label) ->
    COCO rows, with the reference's pre / inference / NMS timing split — against the rows the REFERENCE's own deploy model +
    non_max_suppression + Evaler.convert_to_coco_format produced for the same seeded uint8 batches (tools/make_golden_eval.py, fp32 on the CPU).
    fp32 engine: same images, categories and order; boxes within 5e-3 px of the rescaled coordinates (3-decimal rounding), scores within 2e-5."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_golden_eval as G
    g = golden("eval_loop")
    m = M.Model("n")
    m.load_state_dict(O.synth_state_dict("n", 0, cls_bias=-3.0))
    m = m.to(DEV)
    loop = M.EvalLoop(m, conf_thres=0.03, iou_thres=0.65, half=False, ids=G.COCO_IDS, fold_preprocess=fold)
    res = loop.predict_model(G.batches())
    assert len(res) == int(g["counts"].sum()) == 1500
    assert [r["image_id"] for r in res] == g["image_id"].tolist()
    same_cat = np.asarray([r["category_id"] for r in res]) == g["category_id"]
    bbox = np.asarray([r["bbox"] for r in res]); score = np.asarray([r["score"] for r in res])
    # rows whose scores tie to within fp32 noise may swap places: compare row-wise where the category agrees, and bound the rest
    assert same_cat.mean() >= 0.995, same_cat.mean()
    assert np.abs(bbox[same_cat] - g["bbox"][same_cat]).max() <= 5e-3 + 1e-5 * np.abs(g["bbox"]).max()
    assert np.abs(score[same_cat] - g["score"][same_cat]).max() <= 2e-5
    sp = loop.eval_speed()
    assert set(sp) == {"pre-process", "inference", "NMS"} and all(v >= 0 for v in sp.values()) and loop.speed_result[0].item() == 5
    # the benchmarked precision (half=True, the reference's --half): same loop, detections of the fp16 class
    loop16 = M.EvalLoop(m, conf_thres=0.03, iou_thres=0.65, half=True, ids=G.COCO_IDS, fold_preprocess=fold)
    res16 = loop16.predict_model(G.batches())
    assert len(res16) == 1500
    from nms_cases import match_detections       # same-class, IoU >= 0.95, |d score| <= 1e-2, one-to-one

    def rows_of(img, ids_, cats, boxes, scores):
        k = np.asarray(ids_) == img
        bx = np.asarray(boxes)[k]
        return np.concatenate([bx[:, :2], bx[:, :2] + bx[:, 2:], np.asarray(scores)[k][:, None], np.asarray(cats)[k][:, None].astype(np.float64)], 1)
    matched = 0
    for img in sorted(set(g["image_id"].tolist())):
        ref_rows = rows_of(img, g["image_id"], g["category_id"], g["bbox"], g["score"])
        got_rows = rows_of(img, [r["image_id"] for r in res16], [r["category_id"] for r in res16], [r["bbox"] for r in res16], [r["score"] for r in res16])
        pairs, miss, extra = match_detections(got_rows, ref_rows)
        matched += len(pairs)
    print("fp16 eval loop: %d / 1500 reference rows matched" % matched)
    assert matched >= 1460, matched                        # measured 1481: twice the misses


@pytest.mark.parametrize("thr,frac", [(0.6, (3, 5)), (0.3, (3, 10)), (0.7, (7, 10)), (0.45, (9, 20))])
def test_nms_iou_rule_cpu_vs_cuda_kernel_of_torchvision(thr, frac):
    """on a GPU the reference reaches torchvision's CUDA nms kernel (yolov6/utils/nms.py:96), which compares the fp32 IoU with
    a FLOAT threshold; its CPU kernel (the oracle's and the fixtures' rule, the default here) compares with the double.  They differ exactly
    when the fp32 IoU equals fl32(thr) and fl32(thr) > thr: 0.6 and 0.3 (a pair at IoU 3/5 or 3/10 is suppressed by the CPU rule, kept by the
    CUDA rule); 0.7 and 0.45 round down, no difference.  Both rules are selectable (iou_rule=) and both match the oracle's restatement."""
    num, den = frac
    # box B nested in box A with area ratio num/den: IoU = num/den exactly, fp32 quotient = fl32(thr)
    A = [50.0, 50.0, 50.0 + den, 60.0]; Bx = [50.0, 50.0, 50.0 + num, 60.0]
    rs = np.random.RandomState(int(thr * 100))
    n, nc = 300, 2
    xy = rs.randint(0, 12, (n, 2)).astype(np.float32) * 4 + 200
    wh = rs.randint(1, 7, (n, 2)).astype(np.float32) * 8
    boxes = np.concatenate([xy, xy + wh], 1)
    boxes[0], boxes[1] = A, Bx
    xywh = np.concatenate([(boxes[:, :2] + boxes[:, 2:]) / 2, boxes[:, 2:] - boxes[:, :2]], 1).astype(np.float32)
    cls = (0.2 + 0.7 * rs.rand(n, nc)).astype(np.float32)
    cls[0] = [0.99, 0.001]; cls[1] = [0.98, 0.001]
    pred = np.concatenate([xywh, np.ones((n, 1), np.float32), cls], 1)[None]
    t = torch.from_numpy(pred).to(DEV)
    res = {}
    for rule in ("cpu", "cuda"):
        got, gidx = M.non_max_suppression(t, 0.25, thr, multi_label=True, max_det=1000, return_index=True, iou_rule=rule)
        want, widx = O.non_max_suppression(pred, 0.25, thr, multi_label=True, max_det=1000, return_index=True, float_threshold=(rule == "cuda"))
        assert np.array_equal(gidx[0].cpu().numpy(), widx[0]) and np.array_equal(got[0].cpu().numpy(), want[0]), rule
        res[rule] = set(gidx[0].cpu().tolist())
    b_flat = 1 * nc + 0                                        # candidate (box 1, class 0)
    differs = float(np.float32(thr)) > thr
    assert (b_flat in res["cuda"]) and ((b_flat in res["cpu"]) != differs)
    assert (res["cpu"] != res["cuda"]) == differs or not differs


def test_config4_m_bs1_640_hipgraph_latency_path(models):
    """BASELINE configs[4]: MAF-YOLO-m, bs = 1, 640 x 640, forward replayed from a captured hipGraph + NMS: the replay gives the eager bits,
    the fp32 plan meets the oracle at 1e-3, and the detections of the replayed fp16 prediction equal the oracle's NMS of that prediction."""
    m = models["m"]
    x32 = O.synth_images(1, 640, 3).to(DEV)
    x = x32.half()
    with torch.no_grad():
        eager = m(x)[0].clone()
        plan = m.plan_for(x)
        pred = torch.empty_like(eager)
        for _ in range(3):
            plan.run_into(x, pred, graph=True)
        torch.cuda.synchronize()
        p32 = m(x32)[0]
    assert pred.shape == (1, 8400, 85) and torch.equal(pred, eager)
    kinds = [o.kind for o in plan.ops]
    assert kinds.count(8) == 1                               # P3 (256 wide, 6400 anchors) takes the fused tail; the 384-wide levels keep convs + decode
    ref = O.predict(O.reparam(O.synth_state_dict("m", 0), "m"), "m", x32.cpu()).numpy()
    # fp32 plan vs oracle: m is 151 convs deep and the two fp32 chains sum in different orders; at 640 one box coordinate of 33600 reaches
    # 1.2e-3 px (rel 1e-4): bar 2e-3 px here (1e-3 for n / s and for m at 320, above)
    np.testing.assert_allclose(p32.cpu().numpy()[..., :4], ref[..., :4], rtol=1e-5, atol=2e-3)
    np.testing.assert_allclose(p32.cpu().numpy()[..., 4:], ref[..., 4:], rtol=0, atol=2e-5)
    _close16(pred.cpu().numpy(), ref, "m")
    dets, idx = M.non_max_suppression(pred, 0.03, 0.65, multi_label=True, return_index=True)
    odets, oidx = O.non_max_suppression(pred.cpu().numpy(), 0.03, 0.65, multi_label=True, return_index=True)
    assert np.array_equal(dets[0].cpu().numpy(), odets[0]) and np.array_equal(idx[0].cpu().numpy(), oidx[0])


def test_config4_tuned_bs1_plan_matches_oracle():
    """The plan `bench.py --latency` times since round 6: m, bs = 1, 640 x 640 with `autotune` on (fusion choices and tiles timed for THIS batch size — split-K,
    DMA-ring and pair-input variants that the batch-32 plans never pick).  Its prediction meets the oracle at the fp16 bar, the hipGraph replay gives the eager
    bits, and its detections equal the oracle's NMS of that prediction."""
    m = M.Model("m")
    m.load_state_dict(O.synth_state_dict("m", 0))
    m = m.to(DEV).eval()
    m.autotune = True
    x32 = O.synth_images(1, 640, 3)
    x = x32.to(DEV).half()
    with torch.no_grad():
        plan = m.plan_for(x)
        eager = torch.empty(1, plan.A, 85, dtype=torch.float32, device=DEV)
        plan.run_into(x, eager)
        pred = torch.empty_like(eager)
        for _ in range(3):
            plan.run_into(x, pred, graph=True)
        torch.cuda.synchronize()
    names = [plan.kernel_name(i) for i in range(len(plan.ops))]
    assert any("stream_lds" in n_ or "true" in n_ for n_ in names), "the tuner changed nothing: is autotune on?"
    assert torch.equal(pred, eager)
    ref = O.predict(O.reparam(O.synth_state_dict("m", 0), "m"), "m", x32).numpy()
    _close16(pred.cpu().numpy(), ref, "m")
    dets, idx = M.non_max_suppression(pred, 0.03, 0.65, multi_label=True, return_index=True)
    odets, oidx = O.non_max_suppression(pred.cpu().numpy(), 0.03, 0.65, multi_label=True, return_index=True)
    assert np.array_equal(dets[0].cpu().numpy(), odets[0]) and np.array_equal(idx[0].cpu().numpy(), oidx[0])


def test_bench_line_contract(tmp_path):
    """`python bench.py` prints ONE JSON line with the fields the driver reads (metric, value, unit, n_gpus, steps, warmup, ms_per_step,
    higher_is_better, scaling, vs_baseline, dtype, data, config.workload) plus the roofline object of the dominant kernel; a short run at
    batch 8 without tuning or the CPU leg.  `--dump-outputs` leaves the last timed step's detections, one float32 array per image."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = str(tmp_path / "outputs")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", "8", "--steps", "6", "--warmup", "3", "--no-cpu-baseline", "--no-autotune",
                          "--dump-outputs", dump], cwd=root, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 3 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "images/s" and d["dtype"] == "f16" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 8 * 6 / (d["ms_per_step"] * 6 / 1e3)) / d["value"] < 0.02
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert d["cpu_baseline"] is None                                  # --no-cpu-baseline
    # round 6: NMS alone on the timed head (all-pairs path, both forms) and on an 80-class spread of the same candidates (per-class path); the parity bar of the timed plan
    assert d["ranks_seen"] == 1 and "2e-3" in d["parity_bar_of_the_timed_plan"]
    n = d["nms"]
    assert n["synthetic_head"]["ms_per_batch"] > 0 and n["synthetic_head"]["matrix_form_ms_per_batch"] > 0 and n["classes_spread_80"]["ms_per_batch"] > 0
    assert n["classes_spread_80"]["images_on_per_class_path"] == 8 and n["synthetic_head"]["candidates_per_image"] == n["classes_spread_80"]["candidates_per_image"]
    assert sorted(os.listdir(dump)) == ["detections_%03d.npy" % i for i in range(8)]
    rows = [np.load(os.path.join(dump, "detections_%03d.npy" % i)) for i in range(8)]
    assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 6 and a.shape[0] <= 300 for a in rows)
    a = np.concatenate(rows)
    assert a.shape[0] > 0 and np.isfinite(a).all() and (a[:, 2] >= a[:, 0]).all() and (a[:, 3] >= a[:, 1]).all()
    assert (a[:, 4] > 0.0299).all() and (a[:, 5] == np.round(a[:, 5])).all() and (0 <= a[:, 5]).all() and (a[:, 5] < 80).all()
