"""fp64 restatement of every op kind of an fp16 launch plan, from the op's MafOp, its plan record (engine.Plan._ops[i], whose `raw` holds the fp32 weights
the packer consumed) and snapshots of the op's source slices: the 1x1 conv over concatenated sources (SRC_DIRECT / SRC_UP2 / SRC_POOL2 / SRC_SUB2, fp16 or fp32
output), the 3x3 stride-2 conv (twin, one-launch MPRep `pool1`), the depth-wise conv (one or two filters per input channel), the stem pair (u8 / f16 / f32
image, optional third conv, optional split second output), the fused bottleneck (with and without the block's closing conv), conv1 + depth-wise, SPPF's
three max-pools and the head tail (decoded through oracle.maf_oracle.decode).

`reference(op, rec, srcs, dev, ...)` returns {output name: (ref, bound, S)}: ref float64 in NHWC over the channels that output's slice holds (the head tail:
its [B, H*W, 5 + nc] rows of pred), bound per element.  S is the same chain evaluated on absolute values — |inputs| x |weights| + |bias| — with every
activation replaced by 1.1 |.| (SiLU, ReLU and the sigmoid are 1.1-Lipschitz and |act(y)| <= |y|), so an error of a pre-activation carries over to the
output scaled by at most 1.1 x |weights| and the chain on S bounds it.

Bound: |got - ref| <= ulp(|ref|) + k * 2^-11 * S per element, ulp of the output type (fp16, or fp32 for out_f32).  Inputs are the fp16 values in the arena
(exact) or the image as the stem converts it (the same fp32 operations, rounded to fp16 once); weights are rounded to fp16 exactly as pack rounds them, so
the reference uses the same numbers; biases stay fp32.  Each fp16 x fp16 product is exact in fp32; a stage adds n of them in fp32 (MFMA, v_dot2,
v_fma_mix, split-K partials) with an error of at most n * 2^-24 * S: 2^-10 S for the longest reductions here (n <= 9 * 1280 < 2^14), 2^-13 S for the
fused kernels (n <= 2048).  The activation is evaluated in fp32 (relative error a few 2^-24).  The last store rounds once: at most one ulp of |ref|.
  * one-stage ops (1x1, 3x3 s2, depth-wise): k = K_CONV = 2 (the accumulation and the activation).
  * fused ops keep the fp16 rounding points of tests/test_gpu_fused_parity.py and test_gpu_kernels.py (`_r16`): each point may land one fp16 step away
    from the kernel's (R16 = 2 units) on top of the 1/4 unit of each fused stage: stem pair 0.25 + 2 + 0.25 (+ 2 + 0.25 with the third conv) -> k = 2.5 / 4.75,
    conv1 + depth-wise -> 2.5, bottleneck -> 4.75, with the closing conv -> 7 (<= 8).
  * SPPF: max-pooling moves fp16 values unchanged: equality (bound = 0 is replaced by the smallest fp16 step so the ratio stays defined).
  * head tail: the class / box logits carry k = 2.5 (two stages, one rounding point) plus 2^-24 of their size (the fp32 logits).  Probabilities: sigmoid' <= 1/4, so |dp| <= e / 4 + 2^-20.  Boxes: the
    DFL expectation E = sum_j p_j j over 17 bins moves by dE = sum_j p_j (j - E) dl_j, so |dE| <= 2 sum_j p_j |j - E| e_j (twice the first order) where
    every e_j < 1/4, else |dE| <= 8 max_j e_j (the mean deviation of a distribution on [0, 16] is at most 8); x and w move by at most stride (|dE_l| + |dE_r| + 2^-15), y and h by the same of t / b (the 2^-15
    cells: fp32 softmax and exp), plus 2^-20 |ref|.

What the bound can see: one wrong weight, tap or source pixel changes an output by that one product, about S / n of a reduction of n products; the bound
is k 2^-11 S, so a single stale element shows where n < 2^11 / k (the depth-wise convs, the 1x1 convs up to about 1000 input channels) and otherwise only
through a block of them — a k-step of 8 to 32 channels, a wrong tile, a missed tail: what the sensitivity test of tests/test_gpu_tuner_candidates.py edits.
"""
import torch
import torch.nn.functional as F

from maf_yolo_amd import lib

K_CONV = 2
R16 = 2
K_STAGE = 0.25


def ulp(x, f32=False):
    """Spacing of the fp16 (fp32) numbers at |x| (subnormal spacing below the normal range)."""
    a = x.abs().clamp_min(2.0 ** -14 if not f32 else 2.0 ** -126)
    e = torch.floor(torch.log2(a))
    return torch.pow(2.0, e - (10 if not f32 else 23))


def bound(ref, S, f32=False, k=K_CONV):
    return ulp(ref, f32) + k * 2.0 ** -11 * S


def _act(y, s, act):
    if act == lib.ACT_NONE:
        return y, s
    if act == lib.ACT_RELU:
        y = y.clamp_min(0)
    elif act == lib.ACT_SILU:
        y = y * torch.sigmoid(y)
    elif act == lib.ACT_SIGMOID:
        y = torch.sigmoid(y)
    else:
        raise ValueError(act)
    return y, 1.1 * s


def _w16(w):
    return w.float().half().double()


def _src(x, mode, H, W):
    """One source slice [B, Hs, Ws, C] (fp16) -> what the consumer reads on its H x W grid, float64."""
    x = x.double()
    if mode == lib.SRC_DIRECT:
        return x
    if mode == lib.SRC_UP2:
        return x.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    if mode == lib.SRC_POOL2:
        B, _, _, C = x.shape
        return x[:, :2 * H, :2 * W].reshape(B, H, 2, W, 2, C).amax((2, 4))
    if mode == lib.SRC_SUB2:                                   # pixel (2y, 2x) of a 2H x 2W source: a 1x1 conv with stride 2
        return x[:, :2 * H:2, :2 * W:2]
    raise ValueError(mode)


def _mm(x, w2d, b, act, sx=None):
    """x [B, H, W, K] @ w2d [N, K]^T + b, and the same chain on absolute values (sx: that of x; |x| for an input)."""
    y = torch.matmul(x, w2d.t()) + b
    s = torch.matmul(x.abs() if sx is None else sx, w2d.abs().t()) + b.abs()
    return _act(y, s, act)


def _r16(y, s):
    """A tensor the kernel stores in fp16 (or keeps in LDS as fp16) between two stages: rounded here at the same point.  The kernel rounds its own,
    slightly different, fp32 value, so the two may land one fp16 step apart: at most 2^-10 max(|y|, 2^-14) <= 2 * 2^-11 max(S, 2^-14).  The chain on
    absolute values goes on with max(S, 2^-14), and every such point adds R16 = 2 units to k."""
    return y.half().double(), s.clamp_min(2.0 ** -14)


def _conv3x3s2(x, w, b, act, H, W, sx=None):
    """3 x 3, stride 2, pad 1 as nine tap products (x [B, Hin, Win, C] float64, w [Cout, C, 3, 3] float64)."""
    B, Hin, Win, C = x.shape
    xp = x.new_zeros(B, 2 * H + 2, 2 * W + 2, C)
    sp = x.new_zeros(B, 2 * H + 2, 2 * W + 2, C)
    hh, ww = min(Hin, 2 * H + 1), min(Win, 2 * W + 1)
    xp[:, 1:1 + hh, 1:1 + ww] = x[:, :hh, :ww]
    sp[:, 1:1 + hh, 1:1 + ww] = (x.abs() if sx is None else sx)[:, :hh, :ww]
    y = b.expand(B, H, W, -1).clone()
    s = b.abs().expand(B, H, W, -1).clone()
    for ky in range(3):
        for kx in range(3):
            wt = w[:, :, ky, kx]
            y += torch.matmul(xp[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2], wt.t())
            s += torch.matmul(sp[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2], wt.abs().t())
    return _act(y, s, act)


def _dw(x, w, b, act, cout, sx=None):
    """Depth-wise k x k, pad k // 2, over x [B, H, W, Cin] float64; Cout = 2 Cin: output channel c reads input channel c mod Cin (the head's cls / reg pair)."""
    sx = x.abs() if sx is None else sx
    if cout != x.shape[-1]:
        x, sx = torch.cat([x, x], -1), torch.cat([sx, sx], -1)
    B, H, W, C = x.shape
    k = w.shape[-1]
    p = k // 2
    xp = x.new_zeros(B, H + 2 * p, W + 2 * p, C)
    sp = x.new_zeros(B, H + 2 * p, W + 2 * p, C)
    xp[:, p:p + H, p:p + W] = x
    sp[:, p:p + H, p:p + W] = sx
    wk = w.reshape(C, k, k)
    y = b.expand(B, H, W, -1).clone()
    s = b.abs().expand(B, H, W, -1).clone()
    for ky in range(k):
        for kx in range(k):
            y += xp[:, ky:ky + H, kx:kx + W] * wk[:, ky, kx]
            s += sp[:, ky:ky + H, kx:kx + W] * wk[:, ky, kx].abs()
    return _act(y, s, act)




def _stem_input(x, in_dtype):
    """The image as the stem kernels read it: [B, 3, H, W] -> NHWC fp16 values (u8: x / 255 in fp32, rounded; f32: rounded; f16: as is), float64."""
    if in_dtype == lib.U8:
        x = (x.float() * (1.0 / 255.0)).half()
    else:
        x = x.half()
    return x.permute(0, 2, 3, 1).double()


def _stem1_input(x, in_dtype):
    """The image as the single stem conv (csrc/stem.hip) reads it: [B, 3, H, W] -> NHWC in fp32, never rounded to fp16 (u8: x * (1 / 255) in fp32), float64."""
    x = x.float()
    if in_dtype == lib.U8:
        x = x * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    return x.permute(0, 2, 3, 1).double()


def _out(ref, S, k, f32=False):
    return ref, bound(ref, S, f32, k), S


def reference(op, rec, srcs, dev, twin_src=None, image=None):
    """srcs: the op's source slices as NHWC fp16 tensors [B, Hs, Ws, C_k] on `dev` (for SRC_PAIRS: already turned back into NHWC); twin_src: the twin's;
    image: the stem's [B, 3, Hin, Win] input tensor."""
    kind = op.kind
    raw = [t.to(dev) for t in rec.get("raw", ()) if t is not None and torch.is_tensor(t)]
    f32 = op.dtype == lib.F32                                  # an fp32 launch (the edge suite; the plans are fp16) stores fp32: its ulp
    if kind == lib.OP_STEM:                                    # fp32 weights and fp32 arithmetic on the image as loaded: 27 products
        w, b = raw[:2]
        return {"out": _out(*_conv3x3s2(_stem1_input(image, op.in_dtype), w.double(), b.double(), lib.ACT_RELU, op.H, op.W), K_CONV, f32)}
    if kind == lib.OP_CONV1X1:
        w, b = raw[:2]
        x = torch.cat([_src(s, op.src[k].mode, op.H, op.W) for k, s in enumerate(srcs)], -1)
        return {"out": _out(*_mm(x, _w16(w.reshape(w.shape[0], -1)), b.double(), op.act), K_CONV, bool(op.out_f32) or f32)}
    if kind == lib.OP_CONV3X3S2:
        w, b = raw[:2]
        out = {"out": _out(*_conv3x3s2(srcs[0].double(), _w16(w), b.double(), op.act, op.H, op.W), K_CONV, f32)}
        if rec.get("pool1"):
            w1, b1 = (t.to(dev) for t in rec["pool1"])
            out["pool"] = _out(*_mm(_src(srcs[0], lib.SRC_POOL2, op.H, op.W), _w16(w1.reshape(w1.shape[0], -1)), b1.double(), lib.ACT_SILU), K_CONV)
        if rec.get("twin"):
            w2, b2 = (t.to(dev) for t in rec["twin"]["raw"])
            out["twin"] = _out(*_conv3x3s2(twin_src.double(), _w16(w2), b2.double(), op.act, op.H, op.W), K_CONV, f32)
        return out
    if kind == lib.OP_DWCONV:
        w, b = raw
        return {"out": _out(*_dw(srcs[0].double(), _w16(w), b.double(), op.act, op.Cout), K_CONV, f32)}
    if kind == lib.OP_SPPF_POOL:
        x = srcs[0].double().permute(0, 3, 1, 2)
        ys = []
        for _ in range(3):
            x = F.max_pool2d(x, 5, 1, 2)
            ys.append(x)
        ref = torch.cat(ys, 1).permute(0, 2, 3, 1)
        return {"out": (ref, ulp(ref) * 2.0 ** -11, ref.abs())}
    if kind == lib.OP_STEM2:
        w0, b0, w1, b1 = raw[:4]
        x = _stem_input(image, op.in_dtype)
        H0, W0 = (op.Hin - 1) // 2 + 1, (op.Win - 1) // 2 + 1
        t, s = _r16(*_conv3x3s2(x, _w16(w0), b0.double(), lib.ACT_RELU, H0, W0))
        y, s = _conv3x3s2(t, _w16(w1), b1.double(), lib.ACT_RELU, op.H, op.W, s)
        k = K_STAGE + R16 + K_STAGE
        if op.nc:
            w3, b3 = raw[4:6]
            y, s = _mm(*_r16(y, s)[:1], _w16(w3.reshape(w3.shape[0], -1)), b3.double(), lib.ACT_SILU, _r16(y, s)[1])
            k += R16 + K_STAGE
        if op.aux[0]:                                          # split second output: the upper half of the channels in a tensor of its own
            h = op.Cout // 2
            return {"out": _out(y[..., :h], s[..., :h], k), "out2": _out(y[..., h:], s[..., h:], k)}
        return {"out": _out(y, s, k)}
    if kind in (lib.OP_CONV1DW, lib.OP_BOTTLENECK):
        w1, b1, wd, bd = raw[:4]
        x = srcs[0].double()
        t, s = _r16(*_mm(x, _w16(w1.reshape(w1.shape[0], -1)), b1.double(), lib.ACT_SILU))
        y, s = _dw(t, _w16(wd), bd.double(), lib.ACT_SILU, wd.shape[0], s)
        k = K_STAGE + R16 + K_STAGE
        if kind == lib.OP_CONV1DW:
            return {"out": _out(y, s, k)}
        w2, b2 = raw[4:6]
        y, s = _mm(*_r16(y, s)[:1], _w16(w2.reshape(w2.shape[0], -1)), b2.double(), lib.ACT_SILU, _r16(y, s)[1])
        k += R16 + K_STAGE
        if op.nc:                                              # + the block's closing conv over cat(slots in front, the bottleneck's input, y)
            w3, b3 = raw[6:8]
            yq, sq = _r16(y, s)
            xs = [t_.double() for t_ in srcs[1:]] + [srcs[0].double()]
            xcat = torch.cat(xs + [yq], -1)
            scat = torch.cat([t_.abs() for t_ in xs] + [sq], -1)
            y, s = _mm(xcat, _w16(w3.reshape(w3.shape[0], -1)), b3.double(), lib.ACT_SILU, scat)
            k += R16 + K_STAGE
        return {"out": _out(y, s, k)}
    if kind == lib.OP_HEADTAIL:
        return {"out": _head_tail(op, raw, srcs)}
    raise NotImplementedError("op kind %d" % kind)


def _head_tail(op, raw, srcs):
    from oracle import maf_oracle as O
    B, H, W = op.B, op.H, op.W
    stride = float(op.lvl_stride[0])
    nreg = 4 * (op.reg_max + 1)
    logits = []
    for br, (w1, b1, w2, b2) in enumerate((raw[0:4], raw[4:8])):
        t, s = _r16(*_mm(srcs[br].double(), _w16(w1.reshape(w1.shape[0], -1)), b1.double(), lib.ACT_SILU))
        y, s = _mm(t, _w16(w2.reshape(w2.shape[0], -1)), b2.double(), lib.ACT_NONE, s)
        logits.append((y, (K_STAGE + R16 + K_STAGE) * 2.0 ** -11 * s + 2.0 ** -24 * y.abs()))
    (lc, ec), (lr, er) = logits
    assert lc.shape[-1] == op.nc and lr.shape[-1] == nreg
    cls = torch.sigmoid(lc)
    ref = O.decode([(torch.zeros(B, 1, H, W, dtype=torch.float64), cls.permute(0, 3, 1, 2).cpu(), lr.permute(0, 3, 1, 2).cpu())], strides=(stride,))
    # propagated bound
    r = lr.reshape(B, H * W, 4, op.reg_max + 1)
    e = er.reshape(B, H * W, 4, op.reg_max + 1)
    p = torch.softmax(r, -1)
    j = torch.arange(op.reg_max + 1, dtype=torch.float64, device=r.device)
    E = (p * j).sum(-1, keepdim=True)
    em = e.amax(-1)
    # first order, doubled, where every logit error of the side is below 1/4; else the bound that holds for any size: along the path from the
    # kernel's logits to the reference's, dE/dt <= max_j e_j * sum_j p_j |j - E| <= max_j e_j * reg_max / 2 (mean deviation on [0, reg_max])
    dE = torch.where(em < 0.25, 2 * (p * (j - E).abs() * e).sum(-1), em * op.reg_max / 2).clamp_max(op.reg_max) + 2.0 ** -15     # [B, HW, 4]  l, t, r, b
    bx = (dE[..., 0] + dE[..., 2]) * stride
    by = (dE[..., 1] + dE[..., 3]) * stride
    bnd = torch.empty(B, H * W, 5 + op.nc, dtype=torch.float64, device=r.device)
    bnd[..., 0], bnd[..., 2], bnd[..., 1], bnd[..., 3] = bx, bx, by, by
    bnd[..., 4] = 2.0 ** -24
    bnd[..., 5:] = ec.reshape(B, H * W, op.nc) / 4 + 2.0 ** -20
    ref = ref.to(r.device)
    bnd += 2.0 ** -20 * ref.abs()
    return ref, bnd, None
