"""Training-mode BatchNorm2d (+ residual, + activation), forward and backward, restated in plain fp64 torch on the CPU: the reference of
tests/test_gpu_bn_stats.py for csrc/bn_act.hip, csrc/bn_sum.hip and the statistics epilogues of the conv / depth-wise kernels.

Everything works on rows: x is [M, C] (M = B * H * W pixels), the values the kernel READS — the stored fp16 / fp32 numbers, converted exactly to fp64.
Mean and BIASED variance are the two-pass fp64 ones (mean first, then the mean of the squared deviations): no cancellation whatever |mean| / std is.

    xhat = (x - mean) * rstd,  rstd = 1 / sqrt(var + eps)        u = xhat * gamma + beta [+ residual]        y = act(u)
    g = dz * act'(u)    dbeta = sum g    dgamma = sum g * xhat    dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat))    dresidual = g
    running_mean = (1 - momentum) * running_mean + momentum * mean
    running_var  = (1 - momentum) * running_var  + momentum * var * M / (M - 1)        (M = 1: the biased value, as bn_apply_kernel documents;
                                                                                         torch raises for one value per channel)

fp16 cases: `store` rounds y / dx / dresidual to fp16 as the last step, so a bar on |got - ref| measures the kernel's arithmetic and not the storage format."""
import torch

BARS = {                                                                           # the bars of tests/test_gpu_train.py::test_bn_act_forward_backward
    torch.float32: dict(y=2e-4, grad=4e-4, stat=1e-4),
    torch.float16: dict(y=1e-2, grad=2e-2, stat=2e-3),
}


def rows(t):
    """NCHW-shaped tensor (any strides) -> its [B*H*W, C] rows in fp64 on the CPU"""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu()


def as_nchw(r2d):
    """[M, Cw] rows (contiguous) -> the [1, Cw, 1, M] NHWC view of the same memory (what train_ops.nhwc takes without a copy, also for M = 1)"""
    M, Cw = r2d.shape
    return r2d.view(1, 1, M, Cw).permute(0, 3, 1, 2)


def _act(u, act):
    if act == "silu":
        return u * torch.sigmoid(u)
    if act == "relu":
        return torch.clamp(u, min=0)
    return u


def _act_grad(u, act):
    if act == "silu":
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if act == "relu":
        return (u > 0).double()
    return torch.ones_like(u)


def store(t, dtype):
    return t.to(dtype).double() if dtype == torch.float16 else t


def moments(x):
    """two-pass fp64 mean and biased variance per channel of rows x [M, C]"""
    x = x.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var


def bn_ref(x, gamma, beta, eps, act=None, residual=None, dz=None, momentum=None, running_mean=None, running_var=None, dtype=torch.float32):
    """dict of fp64 tensors: mean, var, rstd, y [, running_mean, running_var] [, dx, dgamma, dbeta, dres].  x, residual, dz: rows [M, C]."""
    x, gamma, beta = x.double(), gamma.double().cpu(), beta.double().cpu()
    M = x.shape[0]
    mean, var = moments(x)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    u = xh * gamma + beta
    if residual is not None:
        u = u + residual.double()
    out = dict(mean=mean, var=var, rstd=rstd, y=store(_act(u, act), dtype))
    if momentum is not None:
        unb = var * M / (M - 1) if M > 1 else var
        out["running_mean"] = (1 - momentum) * running_mean.double().cpu() + momentum * mean
        out["running_var"] = (1 - momentum) * running_var.double().cpu() + momentum * unb
    if dz is not None:
        g = dz.double() * _act_grad(u, act)
        out["dbeta"] = g.sum(0)
        out["dgamma"] = (g * xh).sum(0)
        out["dx"] = store(gamma * rstd * (g - g.mean(0) - xh * (g * xh).mean(0)), dtype)
        out["dres"] = store(g, dtype)
    return out


def err_max(got, ref):
    """max |got - ref| / max |ref| (an all-zero reference: the absolute error)"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    d = float((got - ref).abs().max())
    s = float(ref.abs().max())
    return d / s if s > 0 else d


def err_rel(got, ref):
    """max over the channels of |got - ref| / |ref|"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    return float(((got - ref).abs() / ref.abs()).max())


def ladder_rows(M, C, mean, std, dtype, seed):
    """[M, C] rows of a channel-wise Gaussian, stored in `dtype`: channel c has std `std` and mean `mean` * (its own sign) * (1 +- 20 %) — so channels differ
    and a kernel that mixes two up is seen."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    jit = 1 + 0.2 * (2 * torch.rand(C, generator=g) - 1)
    return (torch.randn(M, C, generator=g) * std + mean * sign * jit).to(dtype)
