"""CPU-side checks of the typed LayerNorm (HGT's use_norm): the fp64 reference means what torch.nn.LayerNorm means, the C entries
validate their arguments before any launch, the Python wrappers name their op, the offset-grid inputs do what the GPU tests rely
on, and the layer registers its parameters only with use_norm.  No GPU."""
import ctypes as C

import pytest
import torch

from tests._typed_layer_norm_ref import (offset_grid, one_pass_f32, outside_tolerance, random_params, random_rows, row_types,
                                         two_pass_f32, typed_layer_norm_ref)
from tests.util import row_ladder_ptrs

HET_OK, HET_ERR_INVALID_ARG, HET_ERR_UNSUPPORTED = 0, 1, 3
ENTRIES = ("het_rows_layer_norm", "het_rows_layer_norm_bf16", "het_rows_layer_norm_backward", "het_rows_layer_norm_backward_bf16")


@pytest.mark.parametrize("X", [8, 10, 64])
def test_reference_is_torch_layer_norm_per_type(X):
    """typed_layer_norm_ref equals torch.nn.LayerNorm(X) modules, one per type, applied to the type's rows in fp64 -- values and the
    gradients of a random cotangent."""
    offs = row_ladder_ptrs()
    T, N = offs.numel() - 1, int(offs[-1])
    gamma, beta = (t.double().requires_grad_(True) for t in random_params(T, X, 1))
    y = random_rows(N, X, 2).double().requires_grad_(True)
    go = torch.randn(N, X, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    out, mean, rstd = typed_layer_norm_ref(y, offs, gamma, beta)
    got = torch.autograd.grad(out, [y, gamma, beta], go)
    norms = [torch.nn.LayerNorm(X, eps=1e-5).double() for _ in range(T)]
    y2 = y.detach().clone().requires_grad_(True)
    with torch.no_grad():
        for t, m in enumerate(norms):
            m.weight.copy_(gamma[t])
            m.bias.copy_(beta[t])
    bounds = offs.tolist()
    ref = torch.cat([norms[t](y2[a:b]) for t, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])
    ref.backward(go)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[0], y2.grad, rtol=1e-10, atol=1e-10)
    for t, m in enumerate(norms):
        wg = m.weight.grad if m.weight.grad is not None else torch.zeros(X, dtype=torch.float64)  # (the empty run)
        bg = m.bias.grad if m.bias.grad is not None else torch.zeros(X, dtype=torch.float64)
        torch.testing.assert_close(got[1][t], wg, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(got[2][t], bg, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(mean, y.detach().mean(1))
    torch.testing.assert_close(rstd, (y.detach().var(1, unbiased=False) + 1e-5).rsqrt())


def test_row_types_with_an_empty_run():
    offs = torch.tensor([0, 2, 2, 5])
    assert row_types(offs, 5).tolist() == [0, 0, 2, 2, 2]


def _args():
    from het_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 65536)()
    h = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)  # (never dereferenced: validation runs before any launch)
    return L, buf, h


def test_entries_validate_before_any_launch():
    L, _buf, h = _args()
    off8, off4 = C.c_void_p(h.value + 8), C.c_void_p(h.value + 4)

    def fwd(name, y=h, out=h, X=64, rows=10, gamma=h):
        return getattr(L, name)(h, 3, y, gamma, h, 1e-5, out, None, None, rows, X, None)

    def bwd(name, y=h, go=h, X=64, rows=10, ws=h, nbytes=1 << 20, gy=h):
        return getattr(L, name)(h, 3, y, h, h, h, go, gy, h, h, ws, nbytes, rows, X, None)

    for name in ENTRIES:
        call = bwd if "backward" in name else fwd
        assert call(name, y=None) == HET_ERR_INVALID_ARG, name  # a NULL data pointer
        assert name.encode() in L.het_last_error(), (name, L.het_last_error())
        for X in (6, 2048, 1028, 2):
            assert call(name, X=X) == HET_ERR_UNSUPPORTED, (name, X)
        assert name.encode() in L.het_last_error()
        assert call(name, rows=0) == HET_OK, name  # no rows: nothing to do
    # rows off their alignment: 16 bytes for fp32 rows, 8 for bf16 rows
    assert fwd("het_rows_layer_norm", y=off8) == HET_ERR_UNSUPPORTED
    assert fwd("het_rows_layer_norm", out=off8) == HET_ERR_UNSUPPORTED
    assert fwd("het_rows_layer_norm", gamma=off8) == HET_ERR_UNSUPPORTED
    assert fwd("het_rows_layer_norm_bf16", y=off4) == HET_ERR_UNSUPPORTED
    assert bwd("het_rows_layer_norm_backward", go=off8) == HET_ERR_UNSUPPORTED
    assert bwd("het_rows_layer_norm_backward", gy=off8) == HET_ERR_UNSUPPORTED
    assert bwd("het_rows_layer_norm_backward_bf16", y=off4) == HET_ERR_UNSUPPORTED
    # the forward's statistics come and go together; the backward wants its workspace
    assert L.het_rows_layer_norm(h, 3, h, h, h, 1e-5, h, h, None, 10, 64, None) == HET_ERR_INVALID_ARG
    assert bwd("het_rows_layer_norm_backward", ws=None) == HET_ERR_INVALID_ARG
    assert bwd("het_rows_layer_norm_backward", nbytes=16) == HET_ERR_INVALID_ARG and b"workspace" in L.het_last_error()
    assert L.het_rows_layer_norm(h, 3, h, h, h, 1e-5, h, None, None, 0, 64, None) == HET_OK  # no rows: nothing to do


def test_shape_predicate_and_workspace_query():
    from het_amd import _lib
    import het_amd.kernels as k
    L = _lib.lib()
    for X, ok in ((4, True), (8, True), (100, True), (1024, True), (10, False), (6, False), (2, False), (0, False), (1028, False), (2048, False)):
        assert k.rows_layer_norm_ok(X) == ok, X
    assert L.het_rows_layer_norm_backward_workspace_bytes(0, 3, 64) == 0
    assert L.het_rows_layer_norm_backward_workspace_bytes(10, 3, 6) == -1
    small, big = (L.het_rows_layer_norm_backward_workspace_bytes(n, 4, 64) for n in (1000, 1_940_000))
    assert small == (4 + 4) * 2 * 64 * 4  # ceil(1000 / 256) tiles + one partial tile per type
    assert 0 < big <= 4 * 2 ** 20  # (a few thousand tiles at most, whatever the row count)


def test_wrappers_name_their_op():
    """A wrong dtype, a non-contiguous tensor or a CPU tensor is refused by the wrapper with the op's name (no GPU needed: the checks
    run first)."""
    import het_amd.kernels as k
    from het_amd._lib import HetError
    offs = torch.tensor([0, 4])
    y, g = torch.zeros(4, 8), torch.ones(1, 8)
    cases = [("rows_layer_norm", lambda: k.rows_layer_norm(offs, y, g, g)),
             ("rows_layer_norm", lambda: k.rows_layer_norm(offs, y.double(), g, g)),
             ("rows_layer_norm", lambda: k.rows_layer_norm(offs, torch.zeros(4, 16)[:, ::2], g, g)),
             ("rows_layer_norm_bf16", lambda: k.rows_layer_norm_bf16(offs, y, g, g)),
             ("rows_layer_norm_backward", lambda: k.rows_layer_norm_backward(offs, y, g, torch.zeros(4), torch.zeros(4), y.half())),
             ("rows_layer_norm_backward_bf16", lambda: k.rows_layer_norm_backward_bf16(offs, y, g, torch.zeros(4), torch.zeros(4), y))]
    for name, call in cases:
        with pytest.raises(HetError, match=name + ":"):
            call()


GRID_X = (8, 32, 64, 256)


@pytest.mark.parametrize("X", GRID_X)
def test_offset_grid_tells_two_pass_from_one_pass(X):
    """The conditions the GPU tests' offset-grid case relies on (the model: tests/test_rgat_kink_inputs.py).  On y = 1024 + k, k an
    integer in [-2, 2]: every value, every row sum in any order and every row mean are exact in fp32; the formula evaluated in
    fp32 with deviations from the mean has NO element outside assert_close's tolerance; with E[y^2] - mean^2 more than half of
    the elements are outside it."""
    N = 4097
    y = offset_grid(N, X, 1024, seed=X)
    offs = torch.tensor([0, 1000, 1000, N])
    t = row_types(offs, N)
    gamma, beta = random_params(3, X, 5)
    y64 = y.double()
    assert bool(((y - 1024).abs() <= 2).all()) and bool((y == y.round()).all())
    perm = torch.randperm(X, generator=torch.Generator().manual_seed(1))
    for cols in (y, y.flip(1), y[:, perm]):  # sequential fp32 sums in three orders
        acc = torch.zeros(N)
        for j in range(X):
            acc = acc + cols[:, j]
        assert torch.equal(acc.double(), y64.sum(1))
    mean32 = y.sum(1) / X
    assert torch.equal(mean32.double(), y64.sum(1) / X)  # (X a power of two: the mean is exact too)
    ref, _, _ = typed_layer_norm_ref(y, offs, gamma, beta)
    two, one = two_pass_f32(y, t, gamma, beta), one_pass_f32(y, t, gamma, beta)
    n_two, n_one = outside_tolerance(two, ref), outside_tolerance(one, ref)
    print(f"X={X}: two-pass max error {float((two.double() - ref).abs().max()):.2e}, one-pass {float((one.double() - ref).abs().nan_to_num(9e9).max()):.2e}, "
          f"one-pass outside {100.0 * n_one / ref.numel():.0f} %")
    assert n_two == 0
    assert n_one > ref.numel() // 2


def test_bf16_offset_grid_is_exact_in_bf16():
    y = offset_grid(257, 64, 64, seed=9)
    assert torch.equal(y.to(torch.bfloat16).float(), y)
    assert torch.equal(y.sum(1).double(), y.double().sum(1))


def test_random_rows_are_not_on_a_grid():
    """X = 100 gets ordinary rows (division by 100 is inexact): per-row mean in [-3, 3], std in [0.1, 10]."""
    y = random_rows(4097, 100, 3).double()
    m, s = y.mean(1), y.std(1)
    assert float(m.abs().max()) < 7 and 0.05 < float(s.min()) < 0.2 and 5 < float(s.max()) < 14


def test_layer_registers_norm_parameters_only_with_use_norm():
    from het_amd.layers import HET_HGTLayerHetero
    plain = HET_HGTLayerHetero(3, 4, 16, 32, num_heads=2)
    assert not any(n.startswith("norm_") for n in plain.state_dict()) and not plain.use_norm
    assert sorted(plain.state_dict()) == sorted(["k_linears", "q_linears", "v_linears", "a_linears", "relation_pri", "relation_att",
                                                 "relation_msg", "skip"])
    normed = HET_HGTLayerHetero(3, 4, 16, 32, num_heads=2, use_norm=True)
    sd = normed.state_dict()
    assert tuple(sd["norm_weight"].shape) == (3, 32) and tuple(sd["norm_bias"].shape) == (3, 32)
    assert bool((sd["norm_weight"] == 1).all()) and bool((sd["norm_bias"] == 0).all()) and normed.norm_eps == 1e-5
    assert set(sd) - set(plain.state_dict()) == {"norm_weight", "norm_bias"}


def test_fallback_composition_matches_the_reference_on_cpu():
    """typed_layer_norm off the kernels' ground (CPU tensors; a width of 10): F.layer_norm per run, values and gradients."""
    from het_amd.backend.hgt_fused_layer import typed_layer_norm
    offs = torch.tensor([0, 3, 3, 40, 57])
    for X in (10, 64):
        gamma, beta = (t.requires_grad_(True) for t in random_params(4, X, 7))
        y = random_rows(57, X, 8).requires_grad_(True)
        go = torch.randn(57, X, generator=torch.Generator().manual_seed(2))
        out = typed_layer_norm(y, offs, gamma, beta, 1e-5)
        got = torch.autograd.grad(out, [y, gamma, beta], go)
        from tests._typed_layer_norm_ref import reference_case
        ref = reference_case(y, offs, gamma, beta, go)
        for a, n in zip((out,) + got, ("out", "grad_y", "grad_gamma", "grad_beta")):
            torch.testing.assert_close(a.detach().double(), ref[n], rtol=2e-4, atol=2e-4, msg=lambda m, n=n: f"{n} X={X}: {m}")
