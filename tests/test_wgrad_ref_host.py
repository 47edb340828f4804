"""The weight-gradient references of tests/test_gpu_wgrad_edges.py (tests/wgrad_ref.py) checked on the CPU: against torch.nn.grad.conv2d_weight in float64, against a
literal five-loop restatement, and for what the exact comparison rests on — that one zeroed border pixel moves the reference, and that int_case refuses inputs whose
sums could leave the exactly representable range."""
import pytest
import torch

import wgrad_ref
from wgrad_ref import conv_wgrad_ref, dw_wgrad_ref, int_case, wide_case


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


# B, Hs, Ws, Cin, Cout, k, s
CONV_SHAPES = [(2, 6, 8, 3, 4, 3, 2),       # even sizes: the last row / column of taps 2 falls on the image's edge
               (2, 7, 5, 2, 3, 3, 2),       # odd Hs, Ws
               (3, 5, 1, 2, 2, 3, 2),       # Wo = 1, Ws = 1 < k: taps kx = 0, 2 see only padding
               (2, 2, 2, 2, 3, 3, 2),       # H < k
               (1, 1, 1, 1, 1, 3, 2),       # one pixel
               (2, 7, 5, 3, 2, 1, 2),       # k = 1 s = 2, odd sizes: reads pixel (2 oy, 2 ox)
               (2, 6, 4, 3, 2, 1, 2),       # k = 1 s = 2, even sizes: the last input row / column is never read
               (2, 5, 4, 3, 5, 1, 1)]


@pytest.mark.parametrize("B,Hs,Ws,cin,cout,k,s", CONV_SHAPES)
def test_conv_reference_matches_conv2d_weight_in_float64(B, Hs, Ws, cin, cout, k, s):
    g = _gen(Hs * 10 + Ws)
    x, dy = wide_case((B, Hs, Ws, cin), g), wide_case((B, _out(Hs, k, s), _out(Ws, k, s), cout), g)
    got, S = conv_wgrad_ref(x, dy, k, s)
    assert got.dtype == torch.float64 and got.shape == ((k, k, cout, cin) if k > 1 else (cout, cin))
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, k, k), dy.double().permute(0, 3, 1, 2), stride=s, padding=k // 2)
    refS = torch.nn.grad.conv2d_weight(x.double().abs().permute(0, 3, 1, 2), (cout, cin, k, k), dy.double().abs().permute(0, 3, 1, 2), stride=s, padding=k // 2)
    ref, refS = ref.permute(2, 3, 0, 1), refS.permute(2, 3, 0, 1)
    if k == 1:
        ref, refS = ref[0, 0], refS[0, 0]
    assert float((got - ref).abs().max()) <= 1e-12 * float(refS.max())
    assert float((S - refS).abs().max()) <= 1e-12 * float(refS.max())
    assert bool((S >= got.abs()).all())


@pytest.mark.parametrize("B,H,W,C,k", [(2, 5, 4, 3, 3), (2, 7, 5, 2, 5), (1, 2, 9, 2, 9), (3, 5, 1, 2, 7), (2, 4, 6, 3, 1), (1, 1, 1, 1, 9)])
def test_depthwise_reference_matches_conv2d_weight_in_float64(B, H, W, C, k):
    g = _gen(H * 10 + W + k)
    x, dy = wide_case((B, H, W, C), g), wide_case((B, H, W, C), g)
    got, S = dw_wgrad_ref(x, dy, k)
    assert got.dtype == torch.float64 and got.shape == (C, k * k)
    f = lambda a, b: torch.nn.grad.conv2d_weight(a.permute(0, 3, 1, 2), (C, 1, k, k), b.permute(0, 3, 1, 2), padding=k // 2, groups=C).reshape(C, k * k)
    ref, refS = f(x.double(), dy.double()), f(x.double().abs(), dy.double().abs())
    assert float((got - ref).abs().max()) <= 1e-12 * float(refS.max())
    assert float((S - refS).abs().max()) <= 1e-12 * float(refS.max())


def _five_loops(x, dy, k, s):
    B, Hs, Ws, cin = x.shape
    _, Ho, Wo, cout = dy.shape
    dw = torch.zeros(k, k, cout, cin, dtype=torch.int64)
    xl, dl = x.long().tolist(), dy.long().tolist()
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = s * oy - k // 2 + ky, s * ox - k // 2 + kx
                        if 0 <= iy < Hs and 0 <= ix < Ws:
                            dw[ky, kx] += torch.tensor(dl[b][oy][ox]).view(-1, 1) * torch.tensor(xl[b][iy][ix]).view(1, -1)
    return dw


@pytest.mark.parametrize("k,s", [(3, 2), (1, 2), (1, 1)])
def test_conv_reference_matches_five_loops_on_a_5x4_map(k, s):
    g = _gen(11 + k + s)
    x, dy = int_case((2, 5, 4, 3), g), int_case((2, _out(5, k, s), _out(4, k, s), 2), g)
    got, _ = conv_wgrad_ref(x, dy, k, s, exact=True)
    want = _five_loops(x, dy, k, s)
    assert got.dtype == torch.int64 and torch.equal(got, want if k > 1 else want[0, 0])


@pytest.mark.parametrize("k", [1, 3, 5])
def test_depthwise_reference_matches_five_loops_on_a_5x4_map(k):
    g = _gen(23 + k)
    x, dy = int_case((2, 5, 4, 3), g), int_case((2, 5, 4, 3), g)
    got, _ = dw_wgrad_ref(x, dy, k, exact=True)
    want = torch.zeros(3, k * k, dtype=torch.int64)
    for b in range(2):
        for y in range(5):
            for xx in range(4):
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = y - k // 2 + ky, xx - k // 2 + kx
                        if 0 <= iy < 5 and 0 <= ix < 4:
                            want[:, ky * k + kx] += dy[b, y, xx].long() * x[b, iy, ix].long()
    assert torch.equal(got, want)


def _nonzero(t):
    """int_case values with the zeros moved to 1, so that dropping any single product changes a sum."""
    return torch.where(t == 0, torch.ones_like(t), t)


@pytest.mark.parametrize("k,s", [(3, 2), (1, 2), (1, 1)])
@pytest.mark.parametrize("corner", [(0, 0), (-1, -1), (0, -1)])
def test_one_zeroed_border_pixel_changes_the_conv_reference(k, s, corner):
    g = _gen(5)
    Hs, Ws = 7, 5                                                   # odd: with s = 2 the last row and column are read (pixel 2 oy of k = 1, tap 1 of k = 3)
    x, dy = _nonzero(int_case((2, Hs, Ws, 3), g)), _nonzero(int_case((2, _out(Hs, k, s), _out(Ws, k, s), 2), g))
    ref, _ = conv_wgrad_ref(x, dy, k, s, exact=True)
    x2 = x.clone()
    x2[1, corner[0], corner[1], 2] = 0
    ref2, _ = conv_wgrad_ref(x2, dy, k, s, exact=True)
    d = (ref2 - ref).abs()
    assert int(d.max()) >= 1 and int(d[..., :2].max()) == 0          # only input channel 2 moves
    dy2 = dy.clone()
    dy2[0, corner[0], corner[1], 1] = 0
    ref3, _ = conv_wgrad_ref(x, dy2, k, s, exact=True)
    d = (ref3 - ref).abs()
    assert int(d.max()) >= 1 and int(d[..., 0, :].max()) == 0        # only output channel 1 moves


@pytest.mark.parametrize("k", [1, 3, 9])
def test_one_zeroed_border_pixel_changes_the_depthwise_reference(k):
    g = _gen(6)
    x, dy = _nonzero(int_case((2, 6, 5, 3), g)), _nonzero(int_case((2, 6, 5, 3), g))
    ref, _ = dw_wgrad_ref(x, dy, k, exact=True)
    for t in (x, dy):
        t2 = t.clone()
        t2[1, -1, 0, 1] = 0
        ref2, _ = dw_wgrad_ref(*((t2, dy) if t is x else (x, t2)), k, exact=True)
        d = (ref2 - ref).abs()
        assert int(d[1].max()) >= 1 and int(d[0].max()) == 0 and int(d[2].max()) == 0


def test_int_case_values_and_its_magnitude_condition():
    g = _gen(7)
    t = int_case((4, 9, 9, 8), g, amp=3)
    assert t.dtype == torch.float16 and torch.equal(t, t.round()) and float(t.abs().max()) == 3 and float(t.min()) == -3
    assert len(t.unique()) == 7
    int_case((1, 1, 466033, 1), g, amp=3)                           # 466033 * 9 = 2^22 - 7
    with pytest.raises(AssertionError):
        int_case((1, 1, 466034, 1), g, amp=3)                       # 466034 * 9 = 2^22 + 2
    with pytest.raises(AssertionError):
        int_case((2, 8, 8, 4), g, amp=3, n_terms=2 ** 19)           # the caller's count rules, not the tensor's
    int_case((1, 1, 2 ** 20, 1), g, amp=1)
    with pytest.raises(AssertionError):
        int_case((1, 1, 2 ** 20, 1), g, amp=2)


def test_wide_case_spans_the_binades_in_fp16():
    t = wide_case((64, 64, 8), _gen(8))
    assert t.dtype == torch.float16 and bool(torch.isfinite(t).all())
    a = t.float().abs()
    assert float(a.max()) > 64 and float(a[a > 0].min()) < 2.0 ** -8
    assert wgrad_ref.wide_case((3, 2), _gen(9)).shape == (3, 2)
