"""Plain restatement of the weight gradients of csrc/wgrad.hip (dense convs) and csrc/train_ops.hip / csrc/dw_wgrad_mfma.hip (depth-wise convs), and the inputs
tests/test_gpu_wgrad_edges.py feeds them.  Device-agnostic torch, float64; checked on the CPU by tests/test_wgrad_ref_host.py.

A weight gradient is a sum of products of two fp16 values accumulated in fp32 (MFMA, v_fma_mix_f32, fp32 atomics).  With small-integer inputs (`int_case`) every
product and every partial sum is an integer below 2^24, exactly representable in fp32, so the kernel must return THE integer whatever the order of its pixel chunks,
channel chunks, replicas and atomics: no tolerance, and one dropped, doubled or misplaced pixel, tap or channel moves the result by at least 1.  `int_case` keeps
n_terms * amp^2 below 2^22: two bits of headroom, so that exactness does not depend on how the MFMA aligns its internal adds.  `wide_case` inputs (binades 2^-6 ..
2^6 mixed per element) are for the error bound |got - ref| <= ulp32(ref) + 2 * n_terms * 2^-24 * S, S the same sum over |x| |dy| (tests/op_ref.py's K_CONV = 2: one
unit for the fp32 accumulation in any order, one for the MFMA's internal order).

Each reference is written as one shifted slice pair and one einsum per tap: tap (ky, kx) of a conv with kernel k, stride s, pad k // 2 multiplies output pixel
(oy, ox) with input pixel (s oy - k // 2 + ky, s ox - k // 2 + kx) where that lies inside the image (k = 1, s = 2: pixel (2 oy, 2 ox))."""
import torch


def _tap_range(n_in, n_out, k, s, t):
    """Output indices o in [lo, hi) whose input index s o - k // 2 + t lies in [0, n_in), and the first such input index."""
    p = k // 2
    lo = max(0, -((t - p) // s))                     # ceil((p - t) / s)
    hi = min(n_out, (n_in - 1 + p - t) // s + 1)
    return lo, hi, s * lo - p + t


def _taps(x, dy, k, s):
    """Yields (ky, kx, x slice, dy slice): the pixels of tap (ky, kx) that lie inside the image, aligned."""
    Hs, Ws, Ho, Wo = x.shape[1], x.shape[2], dy.shape[1], dy.shape[2]
    for ky in range(k):
        y0, y1, iy = _tap_range(Hs, Ho, k, s, ky)
        for kx in range(k):
            x0, x1, ix = _tap_range(Ws, Wo, k, s, kx)
            if y1 <= y0 or x1 <= x0:
                yield ky, kx, None, None
                continue
            yield ky, kx, x[:, iy:iy + s * (y1 - y0 - 1) + 1:s, ix:ix + s * (x1 - x0 - 1) + 1:s], dy[:, y0:y1, x0:x1]


def _as_int(t, exact):
    if not exact:
        return t
    r = t.round()
    assert torch.equal(r, t) and float(t.abs().max()) < 2.0 ** 53
    return r.to(torch.int64)


def conv_wgrad_ref(x, dy, k, s, exact=False):
    """x [B, Hs, Ws, Cin], dy [B, Ho, Wo, Cout] NHWC -> (dW, S): tap-major [k, k, Cout, Cin] ([Cout, Cin] for k = 1), float64; S the same sum over |x| |dy|.
    exact = True: dW and S as int64 (integer inputs: float64 sums of integers below 2^53 are exact)."""
    B, Hs, Ws, Cin = x.shape
    Bo, Ho, Wo, Cout = dy.shape
    assert B == Bo and Ho == (Hs + 2 * (k // 2) - k) // s + 1 and Wo == (Ws + 2 * (k // 2) - k) // s + 1
    xd, dd = x.double(), dy.double()
    dw = torch.zeros(k, k, Cout, Cin, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(dw)
    for ky, kx, xs, ds in _taps(xd, dd, k, s):
        if xs is None:
            continue
        dw[ky, kx] = torch.einsum("bhwo,bhwi->oi", ds, xs)
        S[ky, kx] = torch.einsum("bhwo,bhwi->oi", ds.abs(), xs.abs())
    if k == 1:
        dw, S = dw[0, 0], S[0, 0]
    return _as_int(dw, exact), _as_int(S, exact)


def dw_wgrad_ref(x, dy, k, exact=False):
    """Depth-wise k x k, stride 1, zero padding k // 2: x, dy [B, H, W, C] -> (dW [C, k * k], S), float64 (int64 with exact = True)."""
    assert x.shape == dy.shape
    C = x.shape[-1]
    xd, dd = x.double(), dy.double()
    dw = torch.zeros(C, k * k, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(dw)
    for ky, kx, xs, ds in _taps(xd, dd, k, 1):
        if xs is None:
            continue
        dw[:, ky * k + kx] = torch.einsum("bhwc,bhwc->c", ds, xs)
        S[:, ky * k + kx] = torch.einsum("bhwc,bhwc->c", ds.abs(), xs.abs())
    return _as_int(dw, exact), _as_int(S, exact)


def int_case(shape, gen, amp=3, n_terms=None):
    """fp16 tensor of independent integers in [-amp, amp] (drawn on gen's device).  n_terms: the number of products summed into one dW element (B Ho Wo); default
    the tensor's own pixel count, which is that number for dY and at least that number for X."""
    if n_terms is None:
        n_terms = 1
        for d in shape[:-1]:
            n_terms *= d
    assert n_terms * amp * amp < 2 ** 22, "int_case: %d terms of magnitude %d^2 leave less than two bits under 2^24" % (n_terms, amp)
    return torch.randint(-amp, amp + 1, tuple(shape), generator=gen, device=gen.device).to(torch.float16)


def wide_case(shape, gen):
    """randn * 2^randint(-6, 7) per element, rounded to fp16: neighbours many binades apart, so cancellation and the order of the adds matter."""
    v = torch.randn(tuple(shape), generator=gen, device=gen.device)
    e = torch.randint(-6, 7, tuple(shape), generator=gen, device=gen.device)
    return (v * torch.pow(2.0, e.float())).to(torch.float16)
