"""The typed LayerNorm of HGT's use_norm (include/het_amd.h: het_rows_layer_norm) in fp64 with autograd, the inputs its tests share,
and the two fp32 evaluations (two-pass, one-pass) that show what the offset-grid inputs tell apart.  No GPU needed."""
import torch


def row_types(offsets, num_rows):
    """The run of ``offsets`` [T+1] that holds each row (empty runs allowed)."""
    return torch.searchsorted(offsets[1:].contiguous(), torch.arange(num_rows, device=offsets.device), right=True)


def typed_layer_norm_ref(y, offsets, gamma, beta, eps=1e-5):
    """(out, mean, rstd) in fp64, differentiable in y / gamma / beta:
       mean_v = SUM_j y[v,j] / X;  var_v = SUM_j (y[v,j] - mean_v)^2 / X (biased);  rstd_v = (var_v + eps)^-1/2
       out[v,:] = (y[v,:] - mean_v) * rstd_v * gamma[t(v),:] + beta[t(v),:]"""
    y, gamma, beta = y.double(), gamma.double(), beta.double()
    t = row_types(offsets.to(y.device), y.shape[0])
    mean = y.sum(1, keepdim=True) / y.shape[1]
    d = y - mean
    rstd = ((d * d).sum(1, keepdim=True) / y.shape[1] + eps).rsqrt()
    return d * rstd * gamma[t] + beta[t], mean.squeeze(1), rstd.squeeze(1)


def reference_case(y, offsets, gamma, beta, go, eps=1e-5):
    """{"out", "mean", "rstd", "grad_y", "grad_gamma", "grad_beta"} in fp64 for the cotangent ``go`` (inputs taken as they are given:
    bf16 tensors are widened exactly)."""
    y64, g64, b64 = (t.detach().double().requires_grad_(True) for t in (y, gamma, beta))
    out, mean, rstd = typed_layer_norm_ref(y64, offsets, g64, b64, eps)
    gy, gg, gb = torch.autograd.grad(out, [y64, g64, b64], go.detach().double())
    return {"out": out.detach(), "mean": mean.detach(), "rstd": rstd.detach(), "grad_y": gy, "grad_gamma": gg, "grad_beta": gb}


def random_params(T, X, seed):
    """norm_weight ~ U(0.5, 1.5), norm_bias ~ U(-1, 1), different per type (ones and zeros would hide a wrong type index)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(T, X, generator=gen) + 0.5, torch.rand(T, X, generator=gen) * 2 - 1


def random_rows(N, X, seed):
    """Rows with a per-row mean in [-3, 3] and a per-row std in [0.1, 10]."""
    gen = torch.Generator().manual_seed(seed)
    mean = torch.rand(N, 1, generator=gen) * 6 - 3
    std = 0.1 * 100 ** torch.rand(N, 1, generator=gen)
    return mean + std * torch.randn(N, X, generator=gen)


def offset_grid(N, X, base, seed):
    """y = base + k, k integers in [-2, 2]: |mean| >> std, every value and every row sum exact in fp32 (and, for base = 64, in bf16).
    The variance is at most 4 beside a mean^2 of base^2: E[y^2] - mean^2 in fp32 loses it, the mean of squared deviations does not."""
    gen = torch.Generator().manual_seed(seed)
    return float(base) + torch.randint(-2, 3, (N, X), generator=gen).float()


def two_pass_f32(y, t, gamma, beta, eps=1e-5):
    """The formula evaluated in fp32 the way the kernel does: deviations from the mean, then their mean square."""
    y = y.float()
    mean = y.sum(1, keepdim=True) / y.shape[1]
    d = y - mean
    var = (d * d).sum(1, keepdim=True) / y.shape[1]
    return d * torch.rsqrt(var + eps) * gamma[t] + beta[t]


def one_pass_f32(y, t, gamma, beta, eps=1e-5):
    """... with var = E[y^2] - mean^2 in fp32: what a one-pass kernel would compute."""
    y = y.float()
    mean = y.sum(1, keepdim=True) / y.shape[1]
    var = (y * y).sum(1, keepdim=True) / y.shape[1] - mean * mean
    return (y - mean) * torch.rsqrt(var + eps) * gamma[t] + beta[t]


def outside_tolerance(actual, expected, rtol=2e-4, atol=2e-5):
    """Number of elements outside tests/util.py::assert_close's tolerance (NaN counts as outside)."""
    expected = expected.double()
    a = atol * max(1.0, float(expected.abs().max()))
    return int((~((actual.double() - expected).abs() <= a + rtol * expected.abs())).sum())


def assert_bf16_close(name, a, ref):
    """A bf16 tensor rounded once from an fp32 value against its fp64 reference: elementwise 2^-8 |ref| + 1e-5 max|ref| (the rule of
    tests/test_gpu_bf16_ladders.py)."""
    assert a.dtype == torch.bfloat16, f"{name}: {a.dtype}"
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    d = (a - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
    print(f"{name}: max excess over the bf16 bound {float((d - bound).max()):.2e}")
    assert bool((d <= bound).all()), f"{name}: {int((~(d <= bound)).sum())} elements outside 2^-8 |ref| + 1e-5 max|ref|"
