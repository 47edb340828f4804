"""CPU tests of the letterbox layer (maf-yolo_amd/letterbox.py, csrc/letterbox.hip): the host geometry against what the reference's own code
computed (tests/golden/letterbox_cases.npz, tools/make_golden_letterbox.py), the pixel restatement (tests/letterbox_ref.py) on hand-derived
cases, the argument checks of the C-ABI (no GPU needed: they run before anything touches the device) and the torch op's schema / fake kernel."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import letterbox_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import lib

LB = importlib.import_module("maf_yolo_amd.letterbox")     # the module (the package exports its letterbox() function under the same name)


# ---------------------------------------------------------------- geometry vs the reference

def test_letterbox_geometry_equals_reference(golden):
    g = golden("letterbox_cases")["lb"]
    assert len(g) >= 300
    for row in g:
        h, w, nsh, nsw, auto, scaleup, stride = (int(v) for v in row[:7])
        r, nuw, nuh, top, bottom, left, right, dw, dh, li, ti, resized = row[7:]
        got = LB.letterbox_geometry(h, w, (nsh, nsw), bool(auto), bool(scaleup), stride)
        assert got["r"] == r
        assert got["new_unpad"] == (int(nuw), int(nuh)), (h, w, nsh, nsw)
        assert (got["top"], got["bottom"], got["left"], got["right"]) == (top, bottom, left, right), (h, w, nsh, nsw, auto)
        assert got["ret"] == (r, (dw, dh))
        assert LB.letterbox_geometry(h, w, (nsh, nsw), bool(auto), bool(scaleup), stride, return_int=True)["ret"] == (r, (li, ti))
        assert bool(resized) == (got["new_unpad"] != (w, h))


def test_check_img_size_equals_reference(golden):
    for v, s, nh, nw in golden("letterbox_cases")["check_img_size"]:
        assert LB.check_img_size(int(v), int(s)) == [nh, nw]


def test_eval_geometry_equals_reference(golden):
    z = golden("letterbox_cases")
    ev = z["eval"]
    seen = 0
    for key in z.files:
        if not key.startswith("eval_batch_"):
            continue
        bi, img_size = (int(v) for v in key.split("_")[2:])
        hw0 = [tuple(int(v) for v in s) for s in z[key]]
        bs = LB.rect_batch_shape(hw0, img_size, 32, 0.5)
        rows = ev[(ev[:, 0] == bi) & (ev[:, 1] == img_size)]
        for r in rows:
            h0, w0, h, w, bh, bw, top, left, nrz, interp = (int(v) for v in r[2:12])
            assert bs == [bh, bw]
            g = LB.eval_geometry(h0, w0, bs, img_size)
            assert g["load_hw"] == (h, w) and g["shape"] == (bh, bw) and (g["top"], g["left"]) == (top, left)
            assert nrz == (1 if (h, w) != (h0, w0) else 0) and (nrz == 0 or interp == 1)      # only INTER_LINEAR upscales in scope
            assert g["shapes"] == ((h0, w0), ((r[12], r[13]), (r[14], r[15])))
            seen += 1
    assert seen == len(ev) > 100


def test_mixed_auto_batch_raises_value_error():
    g = {LB.letterbox_geometry(h, w, (640, 640), True, True, 32)["shape"] for h, w in [(1080, 1920), (480, 640)]}
    assert len(g) == 2
    with pytest.raises(ValueError, match="different shapes"):
        LB._check_one_shape([LB.letterbox_geometry(h, w, (640, 640), True, True, 32) for h, w in [(1080, 1920), (480, 640)]])


def test_eval_mode_larger_than_img_size_raises():
    with pytest.raises(M.MafError, match="INTER_AREA"):
        LB.eval_geometry(1080, 1920, [384, 640], 640)
    with pytest.raises(M.MafError, match="resize twice"):
        LB.eval_geometry(480, 640, [320, 320], 640)


def test_cpu_frames_raise():
    with pytest.raises(M.MafError, match="no CPU fallback"):
        M.letterbox([torch.zeros(4, 4, 3, dtype=torch.uint8)])
    with pytest.raises(M.MafError):
        M.eval_batch(torch.zeros(2, 4, 4, 3, dtype=torch.uint8))


# ---------------------------------------------------------------- the pixel restatement, by hand

def test_restatement_identity_copy():
    f = R.synth_frame(5, 7, 1)
    assert np.array_equal(R.resize_linear(f, 7, 5), f)


def test_restatement_area_fast_average():
    f = np.arange(16, dtype=np.uint8).reshape(4, 4, 1) * 9
    out = R.resize_linear(f, 2, 2)
    want = np.array([[(0 + 9 + 36 + 45 + 2) >> 2, (18 + 27 + 54 + 63 + 2) >> 2], [(72 + 81 + 108 + 117 + 2) >> 2, (90 + 99 + 126 + 135 + 2) >> 2]])
    assert np.array_equal(out[..., 0], want)


def test_restatement_upscale_2x3_to_4x6_by_hand():
    f = np.array([[10, 20, 200], [50, 0, 255]], np.uint8)[..., None]
    out = R.resize_linear(f, 6, 4)[..., 0]
    # columns: scale 0.5; fx = 0.5 dx - 0.25 -> dx 0: sx -1 -> clamped (0, 0); dx 1: (0, .25); 2: (0, .75); 3: (1, .25); 4: (1, .75); 5: 2.25 -> clamped (2, 0)
    cols = [(0, 2048, 0), (0, 1536, 512), (0, 512, 1536), (1, 1536, 512), (1, 512, 1536), (2, 2048, 0)]
    # rows: fy = 0.5 dy - 0.25 -> dy 0: sy -1, fy .75 (no coefficient clamp: rows 0, 0); 1: (0, .25); 2: (0, .75); 3: (1, .25) -> rows 1, 1
    rows = [(-1, 512, 1536), (0, 1536, 512), (0, 512, 1536), (1, 1536, 512)]
    src = f[..., 0].astype(np.int64)
    for dy, (sy, b0, b1) in enumerate(rows):
        r0, r1 = min(max(sy, 0), 1), min(max(sy + 1, 0), 1)
        for dx, (sx, a0, a1) in enumerate(cols):
            s1x = min(sx + 1, 2)
            S0 = src[r0, sx] * a0 + src[r0, s1x] * a1
            S1 = src[r1, sx] * a0 + src[r1, s1x] * a1
            v = ((((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16) + 2) >> 2
            assert out[dy, dx] == min(max(v, 0), 255), (dy, dx)
    assert out[0, 0] == 10 and out[0, 5] == 200          # clamped corners of a constant-weight edge keep the source value


def test_restatement_letterbox_border_and_channel_order():
    f = R.synth_frame(3, 4, 2)
    out = R.letterbox_pixels(f, (4, 3), 1, 2, 32, 32, color=(1, 2, 3), bgr=True)
    assert out.shape == (3, 32, 32)
    assert (out[0, 0] == 3).all() and (out[1, 0] == 2).all() and (out[2, 0] == 1).all()      # BGR colour (1, 2, 3) lands as R = 3
    assert np.array_equal(out[0, 1:4, 2:6], f[..., 2]) and np.array_equal(out[2, 1:4, 2:6], f[..., 0])
    rgb = R.letterbox_pixels(f, (4, 3), 1, 2, 32, 32, color=(1, 2, 3), bgr=False)
    assert np.array_equal(rgb[0, 1:4, 2:6], f[..., 0]) and (rgb[0, 0] == 1).all()


def test_rescale_restatement_equals_reference(golden):
    z = golden("letterbox_cases")
    off = 0
    for H, W, h0, w0, n in z["rescale_meta"]:
        got = R.rescale((H, W), z["rescale_in"][off:off + n], (h0, w0))
        assert np.array_equal(got, z["rescale_out"][off:off + n])
        off += n


def test_rescale_params_follow_the_reference():
    p = LB.rescale_params((384, 640), [(1080, 1920), (480, 640)])
    assert p.dtype == np.float32 and p.shape == (2, 5)
    assert p[0, 2] == np.float32(1 / 3) and p[0, 3] == 0 and p[0, 4] == np.float32((384 - 1080 / 3) / 2)


# ---------------------------------------------------------------- C-ABI argument checks (no device touched)

def _img(**kw):
    d = dict(ptr=0x1000, pitch=300, h=10, w=100, new_h=10, new_w=100, top=0, left=0)
    d.update(kw)
    return lib.MafLetterboxImage(**d)


@pytest.mark.parametrize("kw,H,W,msg", [
    (dict(ptr=None), 32, 128, "null frame pointer"),
    (dict(), 30, 128, "multiples of 32"),
    (dict(), 32, 100, "multiples of 32"),
    (dict(new_h=40), 32, 128, "exceeds the output"),
    (dict(left=40), 32, 128, "exceeds the output"),
    (dict(pitch=299), 32, 128, "pitch"),
])
def test_c_abi_letterbox_rejects_bad_arguments(kw, H, W, msg):
    L = lib.load()
    tab = (lib.MafLetterboxImage * 1)(_img(**kw))
    col = (C.c_uint8 * 3)(114, 114, 114)
    rc = L.maf_letterbox(tab, None, 1, H, W, col, 1, C.c_void_p(0x2000), None)
    assert rc != 0 and msg in L.maf_last_error().decode()


def test_c_abi_letterbox_rejects_null_out_and_large_b_without_device_table():
    L = lib.load()
    col = (C.c_uint8 * 3)(114, 114, 114)
    tab = (lib.MafLetterboxImage * 1)(_img())
    assert L.maf_letterbox(tab, None, 1, 32, 128, col, 1, None, None) != 0 and "null pointer" in L.maf_last_error().decode()
    big = (lib.MafLetterboxImage * 65)(*[_img() for _ in range(65)])
    assert L.maf_letterbox(big, None, 65, 32, 128, col, 1, C.c_void_p(0x2000), None) != 0 and "imgs_dev" in L.maf_last_error().decode()
    assert C.sizeof(lib.MafLetterboxImage) == 40


def test_c_abi_rescale_rejects_bad_arguments():
    L = lib.load()
    assert L.maf_rescale_boxes(None, C.c_void_p(0x10), 1, 10, 6, C.c_void_p(0x20), 1, None) != 0 and "null pointer" in L.maf_last_error().decode()
    assert L.maf_rescale_boxes(C.c_void_p(0x10), C.c_void_p(0x10), 0, 10, 6, C.c_void_p(0x20), 1, None) != 0 and "bad shape" in L.maf_last_error().decode()
    assert L.maf_rescale_boxes(C.c_void_p(0x10), C.c_void_p(0x10), 1, 10, 3, C.c_void_p(0x20), 1, None) != 0 and "bad shape" in L.maf_last_error().decode()


# ---------------------------------------------------------------- torch op

def test_torch_op_schema_and_fake_kernel():
    from maf_yolo_amd import torch_ops
    ops = torch_ops.load()
    assert "letterbox" in torch_ops.OPS
    s = str(ops.letterbox.default._schema)
    assert s == "mafyolo::letterbox(Tensor[] frames, int H, int W, int[] geometry, int[] color, bool bgr) -> Tensor"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        frames = [torch.empty(1080, 1920, 3, dtype=torch.uint8), torch.empty(720, 1280, 3, dtype=torch.uint8)]
        out = ops.letterbox(frames, 384, 640, [360, 640, 12, 0, 360, 640, 12, 0], [114, 114, 114], True)
        assert tuple(out.shape) == (2, 3, 384, 640) and out.dtype == torch.uint8


def test_torch_op_rejects_cpu_tensors():
    from maf_yolo_amd import torch_ops
    ops = torch_ops.load()
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.letterbox([torch.zeros(4, 4, 3, dtype=torch.uint8)], 32, 32, [4, 4, 0, 0], [114, 114, 114], True)
