"""The fp64 BatchNorm reference of tests/test_gpu_bn_stats.py (tests/bn_ref.py) against torch's own BatchNorm2d + autograd in fp64 on the CPU: the reference the GPU
tests lean on is itself checked, forward and backward, for every activation, with and without a residual, at a large |mean| / std."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref


@pytest.mark.parametrize("act", [None, "relu", "silu"])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mean,std", [(0.4, 1.7), (16, 0.25)])
def test_reference_matches_torch_autograd_in_fp64(act, residual, mean, std):
    M, c = 777, 24
    g = torch.Generator().manual_seed(3)
    x2 = bn_ref.ladder_rows(M, c, mean, std, torch.float32, 3)
    dz2, r2 = torch.randn(M, c, generator=g), torch.randn(M, c, generator=g)
    bn = torch.nn.BatchNorm2d(c, eps=1e-3, momentum=0.03).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5); bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    ref = bn_ref.bn_ref(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, act, r2 if residual else None, dz2, bn.momentum, torch.zeros(c), torch.ones(c))
    x = bn_ref.as_nchw(x2.double().contiguous()).detach().requires_grad_(True)
    r = bn_ref.as_nchw(r2.double().contiguous()).detach().requires_grad_(True)
    u = bn(x) + r if residual else bn(x)
    y = {None: lambda t: t, "relu": F.relu, "silu": F.silu}[act](u)
    y.backward(bn_ref.as_nchw(dz2.double().contiguous()))
    tol = 1e-9                                                                      # fp64 round-off at |mean| / std = 64 (the cancellation costs ~4 digits of 16)
    assert bn_ref.err_max(bn_ref.rows(y), ref["y"]) < tol
    assert bn_ref.err_max(bn_ref.rows(x.grad), ref["dx"]) < tol
    assert bn_ref.err_max(bn.weight.grad, ref["dgamma"]) < tol and bn_ref.err_max(bn.bias.grad, ref["dbeta"]) < tol
    assert bn_ref.err_max(bn.running_mean, ref["running_mean"]) < tol and bn_ref.err_rel(bn.running_var, ref["running_var"]) < tol
    if residual:
        assert bn_ref.err_max(bn_ref.rows(r.grad), ref["dres"]) < tol


def test_fp16_store_rounds_last_and_one_pixel_uses_the_biased_variance():
    x2 = torch.tensor([[1.5, -2.0, 0.25, 7.0]]).half()
    out = bn_ref.bn_ref(x2, torch.ones(4), torch.full((4,), 0.1), 1e-3, "silu", None, torch.ones(1, 4), 0.03, torch.zeros(4), torch.ones(4), torch.float16)
    assert float(out["var"].abs().max()) == 0 and torch.equal(out["running_var"], torch.full((4,), 0.97, dtype=torch.float64))
    assert torch.equal(out["y"], out["y"].half().double()) and float(out["dx"].abs().max()) == 0
    want = torch.tensor(0.1, dtype=torch.float64)
    assert torch.equal(out["y"], (want * torch.sigmoid(want)).half().double().expand(1, 4))
