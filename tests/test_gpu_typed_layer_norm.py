"""The typed LayerNorm kernels (csrc/rows_layer_norm.hip: het_rows_layer_norm / _backward and their bf16 twins) against the fp64
reference of tests/_typed_layer_norm_ref.py on the row ladder of tests/util.py: 12 runs of 1 .. 4097 rows, one of them empty, run
boundaries in the middle of the kernels' 256-row tiles.  Gradients are taken for a random cotangent (under a uniform one the true
grad_y is zero for a uniform gamma) and the affine parameters are random per type (ones and zeros would hide a wrong type index)."""
import functools

import pytest
import torch

from tests._poison import POISON_IDS, POISONS, poisoned
from tests._typed_layer_norm_ref import assert_bf16_close, offset_grid, random_params, random_rows, reference_case
from tests.util import assert_close, row_ladder_ptrs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32_X = (4, 8, 32, 64, 100, 128, 256, 1024)
BF16_X = (8, 32, 64, 128, 256)
GRID_X = (8, 32, 64, 256)
NAMES = ("out", "mean", "rstd", "grad_y", "grad_gamma", "grad_beta")


@functools.lru_cache(maxsize=None)
def _case(X, kind="random", dtype="f32", T=None, eps=1e-5):
    """Inputs (CPU) and the fp64 reference of one shape, computed once and shared: kind "random" (per-row mean in [-3, 3], std in
    [0.1, 10]), "grid" (1024 + k, or 64 + k for bf16: |mean| >> std) or "const" (zero variance).  T None: the row ladder."""
    offs = row_ladder_ptrs() if T is None else torch.tensor([0] + [5 * (i + 1) for i in range(T)]) if T > 1 else torch.tensor([0, 777])
    N, T = int(offs[-1]), offs.numel() - 1
    gamma, beta = random_params(T, X, 11 + X)
    gen = torch.Generator().manual_seed(100 + X)
    if kind == "random":
        y = random_rows(N, X, 7 + X)
    elif kind == "grid":
        y = offset_grid(N, X, 64 if dtype == "bf16" else 1024, 9 + X)
    else:
        y = (torch.randn(N, 1, generator=gen) * 3).expand(N, X).contiguous()
    go = torch.randn(N, X, generator=gen)
    if dtype == "bf16":
        y, go = y.to(BF16), go.to(BF16)
    return offs, y, gamma, beta, go, reference_case(y, offs, gamma, beta, go, eps)


def _run(case, eps=1e-5, save_stats=True, want_y=True):
    import het_amd.kernels as k
    offs, y, gamma, beta, go, _ = case
    bf16 = y.dtype == BF16
    fwd, bwd = (k.rows_layer_norm_bf16, k.rows_layer_norm_backward_bf16) if bf16 else (k.rows_layer_norm, k.rows_layer_norm_backward)
    offs, y, gamma, beta, go = (t.to(DEV) for t in (offs, y, gamma, beta, go))
    out, mean, rstd = fwd(offs, y, gamma, beta, eps, save_stats=save_stats)
    res = {"out": out, "mean": mean, "rstd": rstd}
    if save_stats:
        res["grad_y"], res["grad_gamma"], res["grad_beta"] = bwd(offs, y, gamma, mean, rstd, go, want_y=want_y)
    torch.cuda.synchronize()
    return res


def _check(res, ref, what):
    for n in NAMES:
        if res.get(n) is None:
            continue
        if res[n].dtype == BF16:
            assert_bf16_close(f"{what} {n}", res[n], ref[n])
        else:
            assert res[n].dtype == torch.float32
            assert_close(res[n], ref[n], what=f"{what} {n}")


@pytest.mark.parametrize("X", F32_X)
def test_fp32_on_the_row_ladder(X):
    """Every lane mapping (1 .. 64 lanes per row, 1 and 4 float4s per lane, a width of 100 with 7 of 32 lanes off): out, the saved
    statistics, grad_y and both parameter gradients."""
    case = _case(X)
    _check(_run(case), case[5], f"X={X}")


@pytest.mark.parametrize("T", [1, 3])
def test_fp32_single_run_and_short_runs(T):
    """One run of 777 rows (T = 1), and three runs of 5 rows in one tile's worth of rows."""
    case = _case(64, T=T)
    _check(_run(case), case[5], f"T={T}")


def test_fp32_one_row():
    import het_amd.kernels as k
    X = 32
    gamma, beta = random_params(1, X, 3)
    y, go = random_rows(1, X, 4), torch.randn(1, X, generator=torch.Generator().manual_seed(5))
    offs = torch.tensor([0, 1])
    ref = reference_case(y, offs, gamma, beta, go)
    _check(_run((offs, y, gamma, beta, go, ref)), ref, "one row")
    empty = torch.zeros(0, X, device=DEV)
    out, mean, rstd = k.rows_layer_norm(torch.tensor([0, 0], device=DEV), empty, gamma.to(DEV), beta.to(DEV))
    gy, gg, gb = k.rows_layer_norm_backward(torch.tensor([0, 0], device=DEV), empty, gamma.to(DEV), mean, rstd, empty)
    assert out.shape == (0, X) and gy.shape == (0, X) and not bool(gg.any()) and not bool(gb.any())


@pytest.mark.parametrize("X", [x for x in F32_X if x & (x - 1) == 0])
def test_constant_rows(X):
    """Zero variance: out is beta[t] bitwise for a power-of-two width (the row sums exactly, so every deviation is 0), rstd is
    eps^-1/2 ~ 316 and grad_y stays finite and inside the tolerance."""
    from tests._typed_layer_norm_ref import row_types
    case = _case(X, kind="const")
    offs, _, _, beta = case[:4]
    res = _run(case)
    assert torch.equal(res["out"].cpu(), beta[row_types(offs, int(offs[-1]))])
    assert bool(torch.isfinite(res["grad_y"]).all())
    assert float((res["rstd"].cpu() - 1e-5 ** -0.5).abs().max()) < 0.1
    _check(res, case[5], f"const X={X}")


@pytest.mark.parametrize("X", GRID_X)
def test_offset_grid(X):
    """y = 1024 + k: fails a one-pass variance (tests/test_typed_layer_norm_ref.py shows by how much), passes the two-pass one."""
    case = _case(X, kind="grid")
    _check(_run(case), case[5], f"grid X={X}")


def test_eps_is_honoured():
    case = _case(64, kind="const", eps=1e-3)
    res = _run(case, eps=1e-3)
    assert float((res["rstd"].cpu() - 1e-3 ** -0.5).abs().max()) < 1e-2
    _check(res, case[5], "eps=1e-3")
    case = _case(32, eps=1e-3)
    _check(_run(case, eps=1e-3), case[5], "eps=1e-3 random")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_optional_outputs_change_no_bits(dtype):
    """NULL mean / rstd (the evaluation pass) gives the same out bits; NULL grad_y the same parameter-gradient bits; a second
    backward the same parameter-gradient bits as the first (no float atomics)."""
    case = _case(64, dtype=dtype)
    full = _run(case)
    assert torch.equal(_run(case, save_stats=False)["out"], full["out"])
    no_y = _run(case, want_y=False)
    assert no_y["grad_y"] is None
    again = _run(case)
    for n in ("grad_gamma", "grad_beta"):
        assert torch.equal(no_y[n], full[n]) and torch.equal(again[n], full[n]), n
    assert torch.equal(again["grad_y"], full["grad_y"])


@pytest.mark.parametrize("X", BF16_X)
def test_bf16_on_the_row_ladder(X):
    """bf16 rows: out and grad_y within 2^-8 |ref| + 1e-5 max|ref| of the fp64 reference on the same bf16 inputs, the fp32 outputs
    (statistics, parameter gradients) at the fp32 tolerance."""
    case = _case(X, dtype="bf16")
    res = _run(case)
    assert res["out"].dtype == BF16 and res["grad_y"].dtype == BF16
    _check(res, case[5], f"bf16 X={X}")


def test_bf16_offset_grid():
    case = _case(64, kind="grid", dtype="bf16")
    _check(_run(case), case[5], "bf16 grid")


@pytest.mark.parametrize("X", [10, 6])
def test_fallback_widths(X):
    """Widths the kernels do not take go through the torch composition of typed_layer_norm and match the reference."""
    from het_amd.backend.hgt_fused_layer import typed_layer_norm
    offs = row_ladder_ptrs()
    N, T = int(offs[-1]), offs.numel() - 1
    gamma, beta = random_params(T, X, 1)
    y, go = random_rows(N, X, 2), torch.randn(N, X, generator=torch.Generator().manual_seed(3))
    ref = reference_case(y, offs, gamma, beta, go)
    yd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (y, gamma, beta))
    out = typed_layer_norm(yd, offs.to(DEV), gd, bd, 1e-5)
    out.backward(go.to(DEV))
    _check({"out": out, "grad_y": yd.grad, "grad_gamma": gd.grad, "grad_beta": bd.grad}, ref, f"fallback X={X}")


@pytest.mark.parametrize("X,dtype", [(64, "f32"), (100, "f32"), (32, "bf16")])
def test_autograd_function(X, dtype, monkeypatch):
    """typed_layer_norm on the kernels' ground is one autograd node: values and the three gradients, only the wanted ones, and under
    torch.no_grad() the same out bits with no statistics saved."""
    import het_amd.kernels as k
    from het_amd.backend.hgt_fused_layer import typed_layer_norm
    offs, y, gamma, beta, go, ref = _case(X, dtype=dtype)
    saved = []
    name = "rows_layer_norm_bf16" if dtype == "bf16" else "rows_layer_norm"
    real = getattr(k, name)
    monkeypatch.setattr(k, name, lambda *a, **kw: (saved.append(kw.get("save_stats", True)), real(*a, **kw))[1])
    yd, gd, bd = (t.to(DEV).requires_grad_(True) for t in (y, gamma, beta))
    out = typed_layer_norm(yd, offs.to(DEV), gd, bd, 1e-5)
    out.backward(go.to(DEV))
    _check({"out": out, "grad_y": yd.grad, "grad_gamma": gd.grad, "grad_beta": bd.grad}, ref, f"autograd X={X} {dtype}")
    with torch.no_grad():
        ev = typed_layer_norm(yd, offs.to(DEV), gd, bd, 1e-5)
    assert torch.equal(ev, out) and saved == [True, False]
    y2 = y.to(DEV)  # the input needs no gradient: the parameters still get theirs
    gd.grad = bd.grad = None
    typed_layer_norm(y2, offs.to(DEV), gd, bd, 1e-5).backward(go.to(DEV))
    _check({"grad_gamma": gd.grad, "grad_beta": bd.grad}, ref, "parameters only")


@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
@pytest.mark.parametrize("X,dtype", [(64, "f32"), (100, "f32"), (32, "bf16")])
def test_nothing_uninitialised_is_read(X, dtype, value):
    """With every tensor the wrappers take uninitialised (outputs, statistics, the backward's workspace) filled with NaN or 1e30 first,
    the results are the bits they were: no slot is read before it is written."""
    case = _case(X, dtype=dtype)
    clean = _run(case)
    with poisoned(value) as record:
        dirty = _run(case)
    assert len(record.from_module("het_amd.kernels")) >= 6  # out, mean, rstd, grad_y, two parameter gradients, the workspace
    for n in NAMES:
        assert torch.equal(clean[n], dirty[n]), n
    _check(dirty, case[5], f"poisoned X={X} {dtype}")
