"""The two single-launch parameter entries of the RGAT step (csrc/node_gemm.hip): het_rgat_transpose_weights -- W^T [R,H,D,K] and
loop_w^T [X,K], exact copies -- and het_rgat_unfold_weight_gradient, the gradient through the folded weight wa = W . attn_r."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = list(itertools.product((1, 3, 8), (1, 4), (32, 64), (16, 32)))  # (R, H, K, D)
# max |fp32 torch composition - fp64| / max |fp64| of _unfold_torch over SHAPES, evaluated on the CPU (unfold_deviation_on_cpu below);
# the figures: grad_W 7.6e-8, grad_attn_r 1.5e-7.  The kernel is allowed 4 x that.
UNFOLD_DEVIATION = {"grad_W": 7.6e-8, "grad_attn_r": 1.5e-7}


def _misaligned(t):
    """A contiguous view of the same values whose first element is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("with_loop", [True, False])
@pytest.mark.parametrize("R,H,K,D", SHAPES)
def test_transposes_are_exact_copies(R, H, K, D, with_loop, aligned):
    import het_amd.kernels as k
    torch.manual_seed(R * 1000 + H * 100 + K + D)
    X = H * D
    W = torch.randn(R, H, K, D, device=DEV)
    loop_w = torch.randn(K, X, device=DEV) if with_loop else None
    if not aligned:
        W = _misaligned(W)
        loop_w = None if loop_w is None else _misaligned(loop_w)
    Wt, loop_wt = k.rgat_transpose_weights(W, loop_w)
    torch.cuda.synchronize()
    assert Wt.shape == (R, H, D, K) and Wt.is_contiguous()
    assert torch.equal(Wt, W.transpose(2, 3).contiguous())
    if with_loop:
        assert loop_wt.shape == (X, K) and loop_wt.is_contiguous()
        assert torch.equal(loop_wt, loop_w.t().contiguous())
    else:
        assert loop_wt is None


def test_transposes_of_a_rectangular_self_loop_weight():
    """loop_w [K,X] with X != H*D and K != X (the entry takes X on its own), more than one workgroup per tensor."""
    import het_amd.kernels as k
    torch.manual_seed(0)
    W = torch.randn(5, 2, 48, 24, device=DEV)
    loop_w = torch.randn(48, 136, device=DEV)
    Wt, loop_wt = k.rgat_transpose_weights(W, loop_w)
    assert torch.equal(Wt, W.transpose(2, 3).contiguous()) and torch.equal(loop_wt, loop_w.t().contiguous())


def _unfold_case(R, H, K, D, dtype=torch.float32):
    """(grad_wa [R,H,K,1], W, attn_r, grad_W before the call) on the CPU, in ``dtype`` from one fp32 draw."""
    gen = torch.Generator().manual_seed(R * 1000 + H * 100 + K + D)
    draw = lambda *shape: torch.randn(*shape, generator=gen)
    return tuple(t.to(dtype) for t in (draw(R, H, K, 1), draw(R, H, K, D) * 0.2, draw(R, H, D), draw(R, H, K, D)))


def _unfold_torch(grad_wa, W, attn_r, grad_W):
    """The composition the entry replaces (and, in fp64, its reference): returns (grad_W + grad_wa (x) attn_r, grad_attn_r)."""
    R, H, K, D = W.shape
    return grad_W + grad_wa * attn_r.view(R, H, 1, D), (W * grad_wa).sum(2)


def _rel_dev(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def unfold_deviation_on_cpu():
    """The measured bound: the deviation of the fp32 torch composition from the fp64 one over SHAPES, on the CPU."""
    dev = {"grad_W": 0.0, "grad_attn_r": 0.0}
    for shape in SHAPES:
        got, ref = _unfold_torch(*_unfold_case(*shape)), _unfold_torch(*_unfold_case(*shape, dtype=torch.float64))
        dev["grad_W"] = max(dev["grad_W"], _rel_dev(got[0], ref[0]))
        dev["grad_attn_r"] = max(dev["grad_attn_r"], _rel_dev(got[1], ref[1]))
    return dev


@pytest.mark.parametrize("R,H,K,D", SHAPES)
def test_unfold_weight_gradient(R, H, K, D):
    """Against the same formula in fp64.  Bound: 4 x the deviation of the fp32 torch composition from fp64 on these cases, measured
    on the CPU (UNFOLD_DEVIATION: max |difference| / max |fp64 value|, grad_W 7.6e-8 and grad_attn_r 1.5e-7); the figure is printed
    before it is judged.  Two calls give the same bits (fixed order, no atomics)."""
    import het_amd.kernels as k
    grad_wa, W, attn_r, grad_W0 = _unfold_case(R, H, K, D)
    ref_W, ref_ar = _unfold_torch(*_unfold_case(R, H, K, D, dtype=torch.float64))
    results = []
    for _ in range(2):
        grad_W = grad_W0.to(DEV)
        grad_attn_r = k.rgat_unfold_weight_gradient(grad_wa.to(DEV), W.to(DEV), attn_r.to(DEV), grad_W)
        torch.cuda.synchronize()
        results.append((grad_W.cpu(), grad_attn_r.cpu()))
    (gW, gar), (gW2, gar2) = results
    assert gar.shape == (R, H, D)
    dW, dar = _rel_dev(gW, ref_W), _rel_dev(gar, ref_ar)
    print(f"unfold R={R} H={H} K={K} D={D}: grad_W {dW:.3e} (bound {4 * UNFOLD_DEVIATION['grad_W']:.3e}), "
          f"grad_attn_r {dar:.3e} (bound {4 * UNFOLD_DEVIATION['grad_attn_r']:.3e})")
    assert dW <= 4 * UNFOLD_DEVIATION["grad_W"]
    assert dar <= 4 * UNFOLD_DEVIATION["grad_attn_r"]
    assert torch.equal(gW, gW2) and torch.equal(gar, gar2), "two calls differ"


def test_unfold_weight_gradient_on_misaligned_and_odd_shapes():
    """No alignment is asked of any pointer; D that does not divide the workgroup, K that is no multiple of the slices."""
    import het_amd.kernels as k
    torch.manual_seed(1)
    R, H, K, D = 2, 3, 50, 24
    grad_wa, W, attn_r, grad_W0 = (torch.randn(R, H, K, 1), torch.randn(R, H, K, D) * 0.2, torch.randn(R, H, D), torch.randn(R, H, K, D))
    ref_W, ref_ar = _unfold_torch(grad_wa.double(), W.double(), attn_r.double(), grad_W0.double())
    grad_W = _misaligned(grad_W0.to(DEV))
    gar = k.rgat_unfold_weight_gradient(_misaligned(grad_wa.to(DEV)), _misaligned(W.to(DEV)), _misaligned(attn_r.to(DEV)), grad_W)
    torch.cuda.synchronize()
    assert _rel_dev(grad_W.cpu(), ref_W) <= 4 * UNFOLD_DEVIATION["grad_W"]
    assert _rel_dev(gar.cpu(), ref_ar) <= 4 * UNFOLD_DEVIATION["grad_attn_r"]


def test_measured_bound_is_the_one_written_down():
    """UNFOLD_DEVIATION is what unfold_deviation_on_cpu measures (to the digits written; the CPU's sum order may move the last one)."""
    got = unfold_deviation_on_cpu()
    for n, v in UNFOLD_DEVIATION.items():
        assert 0.5 * v <= got[n] <= 2.0 * v, (n, got[n], v)
