"""The softmax cross-entropy kernels (csrc/softmax_xent.hip) and their autograd node (het_amd/layers.py SoftmaxCrossEntropy) on the
GPU against the numpy fp64 reference of the rule (tests/_softmax_xent_ref.py) on the same (bf16-rounded) logits: the class-count and
row-count ladders around every lane-mapping threshold and the end of a grid's first pass, exact cases, specials, the gradient's scale,
bit determinism, the autograd contract, uninitialised buffers, the torch composition for tensors the kernels do not take, and
agreement with the training script's default expression."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _softmax_xent_ref as ref
from tests._poison import POISON_IDS, POISONS, poisoned
from tests.util import LADDER, ROW_LADDER, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("fp32", "bf16")


def _k():
    import het_amd.kernels as k
    return k


def _thresholds():
    return _k().softmax_xent_thresholds()


def _class_counts():
    t = _thresholds()
    return tuple(sorted(set(LADDER + (349, 1023, 1024, 1025, 4097) + tuple(v + d for v in t for d in (-1, 0, 1)))))


def _row_counts(C):
    p = _k().softmax_xent_rows_per_pass(C)  # rows a full grid takes before a wave takes a second one
    return tuple(ROW_LADDER) + (p - 1, p, p + 1, p + 257)


CLASS_ROWS = (1, 33, 257)          # every class count at these row counts (one row; rows that do not fill a wave; several workgroups)
ROW_CLASSES = (3, 8, 349)          # every row count at these class counts (12-byte rows, one lane per row; 32-byte rows; a wave per row)


def _case(N, C, dtype, seed, ignore_index=-100, ignored=0.25, bad=True, scale=3.0):
    """(logits on the device in `dtype`, the same values fp64 numpy, labels numpy, labels on the device)."""
    rng = np.random.default_rng(seed)
    z = torch.tensor(rng.standard_normal((N, C)) * scale, dtype=torch.float32).to(dtype)
    lab = ref.draw_labels(rng, N, C, ignored=ignored, bad=bad, ignore_index=ignore_index)
    return z.to(DEV), z.double().numpy(), lab, torch.tensor(lab, device=DEV)


def _assert_bf16_close(got, want, what):
    """The project's bf16 rule: elementwise within 2^-8 |ref| + 1e-5 max|ref|."""
    want = np.asarray(want, dtype=np.float64)
    got = got.detach().float().cpu().double().numpy()
    bound = 2.0 ** -8 * np.abs(want) + 1e-5 * float(np.abs(want).max(initial=0.0))
    worst = float((np.abs(got - want) - bound).max(initial=-1.0))
    assert worst <= 0.0, f"{what}: {worst:.3e} beyond the bf16 bound"


def _check(N, C, dtype, seed, reduction, ignore_index=-100):
    """One forward + backward through the wrappers against the reference: loss, lse, stats, gradient."""
    k = _k()
    zd, z64, lab, labd = _case(N, C, dtype, seed, ignore_index)
    loss, lse, stats = k.softmax_xent(zd, labd, ignore_index, reduction)
    want_loss, want_lse, want_stats, _ = ref.forward(z64, lab, ignore_index, reduction)
    what = f"N={N} C={C} {dtype} {reduction}"
    assert stats.dtype == torch.int64 and stats.tolist() == want_stats.tolist(), what
    assert loss.dtype == torch.float32 and loss.dim() == 0 and lse.dtype == torch.float32 and lse.shape == (N,)
    if np.isnan(want_loss):
        assert bool(torch.isnan(loss)), what
    else:
        assert_close(loss, torch.tensor(want_loss), what=what + " loss")
    assert_close(lse, torch.tensor(want_lse), what=what + " lse")
    # the scale 1 / valid and g: g = -2.5 * valid for the mean keeps the gradient's magnitude (and so the tolerance's meaning) at any N
    g = -2.5 * (max(int(want_stats[0]), 1) if reduction == "mean" else 1)
    grad = k.softmax_xent_backward(zd, labd, lse, stats, torch.tensor(g, dtype=torch.float32, device=DEV), ignore_index, reduction)
    assert grad.dtype == dtype and grad.shape == (N, C) and grad.is_contiguous()
    want_grad = ref.backward(z64, lab, want_lse, g, ignore_index, reduction)
    if dtype == torch.float32:
        assert_close(grad, torch.tensor(want_grad), what=what + " grad")
    else:
        _assert_bf16_close(grad, want_grad, what + " grad")
    valid, _ = ref.rows(lab, C, ignore_index)
    skipped = grad[torch.tensor(~valid, device=DEV)].float()
    assert not bool(skipped.any()) and not bool(torch.signbit(skipped).any()), what + ": a skipped row is +0"
    assert not bool(lse[torch.tensor(~valid, device=DEV)].any())
    return want_stats


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_class_count_ladder(dtype):
    counts = _class_counts()
    for t in _thresholds():
        assert {t - 1, t, t + 1} <= set(counts)
    for i, C in enumerate(counts):
        for N in CLASS_ROWS:
            stats = _check(N, C, dtype, 1000 * C + N, ("mean", "sum")[i % 2])
            if N == CLASS_ROWS[-1]:
                assert 0 < stats[0] < N and stats[2] >= 2  # valid, ignored and bad rows


@pytest.mark.parametrize("C", ROW_CLASSES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_row_count_ladder(dtype, C):
    rows = _row_counts(C)
    assert 0 in rows and 1 in rows and max(rows) > _k().softmax_xent_rows_per_pass(C)
    for i, N in enumerate(rows):
        _check(N, C, dtype, 7 * N + C, ("sum", "mean")[i % 2])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_custom_ignore_index_and_all_rows_ignored(dtype):
    k = _k()
    stats = _check(300, 8, dtype, 5, "mean", ignore_index=2)
    assert 0 < stats[0] < 300
    zd, _, _, _ = _case(70, 5, dtype, 6)
    labd = torch.full((70,), -100, device=DEV)
    for reduction in ("mean", "sum"):
        loss, lse, stats = k.softmax_xent(zd, labd, -100, reduction)
        assert stats.tolist() == [0, 0, 0] and not bool(lse.any())
        assert bool(torch.isnan(loss)) if reduction == "mean" else float(loss) == 0.0
        grad = k.softmax_xent_backward(zd, labd, lse, stats, torch.ones((), device=DEV), -100, reduction)
        assert not bool(grad.float().any()) and not bool(torch.signbit(grad.float()).any())  # all +0, not 0 * (1 / 0)
    loss, lse, stats = k.softmax_xent(zd[:0], labd[:0], -100, "mean")  # no rows: no launch
    assert bool(torch.isnan(loss)) and stats.tolist() == [0, 0, 0] and lse.shape == (0,)
    assert float(k.softmax_xent(zd[:0], labd[:0], -100, "sum")[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_equal_logits_give_log_c(dtype):
    k = _k()
    for C in (1, 2, 3, 8, 9, 349, 1025):
        want = np.float32(np.log(np.float64(C)))
        for v in (0.0, 1.5, -96.0):
            z = torch.full((1, C), v, dtype=dtype, device=DEV)
            loss, lse, _ = k.softmax_xent(z, torch.tensor([C // 2], device=DEV), -100, "sum")
            assert abs(np.float64(float(loss)) - np.float64(want)) <= np.spacing(want), (C, v, float(loss), want)
        # the gradient: 1 / C off the label, 1 / C - 1 at it, scaled -- the reference takes lse as the kernel stored it
        N = 37
        vals = torch.tensor([0.0, 1.5, -96.0, 7.0])[torch.arange(N) % 4]
        z = vals[:, None].expand(N, C).contiguous().to(dtype).to(DEV)
        lab = np.arange(N) % C
        labd = torch.tensor(lab, device=DEV)
        loss, lse, stats = k.softmax_xent(z, labd, -100, "mean")
        assert stats.tolist() == [N, int((lab == 0).sum()), 0]  # (all maxima: only label 0 is the first)
        grad = k.softmax_xent_backward(z, labd, lse, stats, torch.tensor(-2.5, device=DEV), -100, "mean")
        want_grad = ref.backward(z.double().cpu().numpy(), lab, lse.double().cpu().numpy(), -2.5, -100, "mean")
        ideal = (np.full((N, C), 1.0 / C) - np.eye(C)[lab]) * (-2.5 / N)
        if dtype == torch.float32:
            # the kernel's exp is the hardware's exp2 of x * log2(e): the product is rounded once (|x| * 2^-24 of the result), exp2, the
            # subtraction and the scaling add an ulp each; x = -log C here
            np.testing.assert_allclose(grad.double().cpu().numpy(), want_grad, rtol=(np.log(C) + 4) * 2.0 ** -23, atol=1e-9)
            assert_close(grad, torch.tensor(ideal), what=f"C={C}")
        else:
            _assert_bf16_close(grad, want_grad, f"C={C} (lse as stored)")
            _assert_bf16_close(grad, ideal, f"C={C}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_logit_far_above_the_rest(dtype):
    k = _k()
    for C in (2, 8, 349):
        N = 19
        lab = (np.arange(N) * 5) % C
        z = torch.zeros(N, C)
        z[torch.arange(N), torch.tensor(lab)] = 1e4
        z = z.to(dtype).to(DEV)
        labd = torch.tensor(lab, device=DEV)
        loss, lse, stats = k.softmax_xent(z, labd, -100, "sum")
        assert float(loss) == 0.0 and stats.tolist() == [N, N, 0] and bool(torch.isfinite(lse).all())
        grad = k.softmax_xent_backward(z, labd, lse, stats, torch.tensor(3.0, device=DEV), -100, "sum")
        assert not bool(grad.float().any())  # exactly 0 off the label (expf underflows) and at it (expf(0) - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_argmax_ties_resolve_to_the_lowest_index(dtype):
    k = _k()
    rng = np.random.default_rng(3)
    for C in (2, 6, 8, 17, 349):
        N = 512
        z64 = rng.integers(-2, 3, size=(N, C)).astype(np.float64)  # exact in bf16; most rows have tied maxima
        s = np.sort(z64, axis=1)
        assert (s[:, -1] == s[:, -2]).sum() > N // 8
        z64[5, C - 1] = np.nan  # a NaN is the maximum
        z64[6, :] = np.nan      # ... and the first of several wins
        lab = rng.integers(0, C, size=N)
        lab[5], lab[6] = C - 1, 0
        am = ref.argmax_first(z64)
        lab[::3] = am[::3]  # (a third of the rows correct for certain)
        zd = torch.tensor(z64, dtype=torch.float32).to(dtype).to(DEV)
        _, _, stats = k.softmax_xent(zd, torch.tensor(lab, device=DEV), -100, "sum")
        assert stats.tolist() == [N, int((am == lab).sum()), 0], C
        assert np.array_equal(am, torch.argmax(torch.tensor(z64), dim=1).numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_specials_match_torch_on_the_cpu_by_class(dtype):
    from het_amd.layers import SoftmaxCrossEntropy
    rows = [(list(r), l) for r, l in ref.SPECIAL_ROWS]
    rows += [(list(r) + [-np.inf] * 9 + [0.25] * 4, l) for r, l in ref.SPECIAL_ROWS]  # the same in rows of 17: several lanes per row
    for r, l in rows:
        z = torch.tensor([r], dtype=torch.float32).to(dtype)
        zt = z.float().clone().requires_grad_(True)
        want = F.cross_entropy(zt, torch.tensor([l]), reduction="sum")
        want.backward()
        zd = z.to(DEV).requires_grad_(True)
        loss = SoftmaxCrossEntropy(reduction="sum")(zd, torch.tensor([l], device=DEV))
        loss.backward()
        assert ref.float_class(loss.item()) == ref.float_class(want.item()), (r, l, loss.item(), want.item())
        np.testing.assert_array_equal(ref.float_class(zd.grad.float().cpu().numpy()), ref.float_class(zt.grad.numpy()), err_msg=str((r, l)))
        if np.isfinite(want.item()):
            assert_close(loss, want.detach(), what=str((r, l)))


# ---------------------------------------------------------------------------------------------- gradient, scale and determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_gradient_scale_and_incoming_gradient(dtype):
    from het_amd.layers import SoftmaxCrossEntropy
    cmp = (lambda a, b, w: assert_close(a, torch.tensor(b), what=w)) if dtype == torch.float32 else _assert_bf16_close
    for reduction in ("mean", "sum"):
        z1, z1_64, lab1, lab1d = _case(301, 8, dtype, 21)
        z2, z2_64, lab2, lab2d = _case(77, 349, dtype, 22)
        mod = SoftmaxCrossEntropy(reduction=reduction)
        a = z1.clone().requires_grad_(True)
        mod(a, lab1d).backward(torch.tensor(-2.5))  # (a CPU scalar: autograd moves it; the kernel reads it on the device)
        _, lse1, _, _ = ref.forward(z1_64, lab1, -100, reduction)
        cmp(a.grad, ref.backward(z1_64, lab1, lse1, -2.5, -100, reduction), "backward(-2.5)")
        # two calls made before either backward: each node keeps its own lse, stats and scale
        a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        l1, l2 = mod(a, lab1d), mod(b, lab2d)
        (3 * l1 + l2).backward()
        _, lse2, _, _ = ref.forward(z2_64, lab2, -100, reduction)
        cmp(a.grad, ref.backward(z1_64, lab1, lse1, 3.0, -100, reduction), "3 * loss1")
        cmp(b.grad, ref.backward(z2_64, lab2, lse2, 1.0, -100, reduction), "+ loss2")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_same_bits_on_every_call(dtype):
    k = _k()
    for N, C in ((4099, 8), (1031, 349), (3001, 3)):
        zd, _, _, labd = _case(N, C, dtype, N + C)
        g = torch.tensor(0.75, device=DEV)
        loss, lse, stats = k.softmax_xent(zd, labd)
        grad = k.softmax_xent_backward(zd, labd, lse, stats, g)
        other = _case(513, 17, dtype, 1)
        k.softmax_xent(other[0], other[3])  # another shape in between: nothing depends on the launch history
        loss2, lse2, stats2 = k.softmax_xent(zd, labd)
        grad2 = k.softmax_xent_backward(zd, labd, lse2, stats2, g)
        assert loss.view(torch.int32).item() == loss2.view(torch.int32).item()
        assert torch.equal(lse, lse2) and torch.equal(stats, stats2) and torch.equal(grad, grad2)


# ------------------------------------------------------------------------------------------------------- the autograd contract
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_autograd_contract(dtype):
    from het_amd.layers import SoftmaxCrossEntropy
    zd, _, _, labd = _case(523, 8, dtype, 31)
    z0, lab0 = zd.clone(), labd.clone()
    mod = SoftmaxCrossEntropy()
    bits = lambda t: t.detach().view(torch.int32).item()  # noqa: E731
    assert not mod(zd, labd).requires_grad  # logits without a gradient: nothing to differentiate
    a = zd.clone().requires_grad_(True)
    train = mod(a, labd)
    assert train.requires_grad and not mod.last_stats.requires_grad
    with torch.no_grad():
        quiet = mod(a, labd)
    with torch.inference_mode():
        inf = mod(a, labd)
        acc = mod.accuracy()
    assert not quiet.requires_grad and bits(quiet) == bits(train) and bits(inf.clone()) == bits(train)
    assert 0.0 <= float(acc) <= 1.0
    train.backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    train.backward()
    assert torch.equal(a.grad, g1)  # the second backward through the retained graph: the same bits
    # returned gradients keep their bits through a second step on other inputs
    other = _case(1025, 17, dtype, 32)
    b = other[0].clone().requires_grad_(True)
    mod(b, other[3]).backward()
    assert torch.equal(a.grad, g1)
    # .grad accumulates over two backwards
    c = zd.clone().requires_grad_(True)
    mod(c, labd).backward()
    mod(c, labd).backward()
    want = (g1.float() * 2).to(dtype)
    assert torch.equal(c.grad, want)
    assert torch.equal(zd, z0) and torch.equal(labd, lab0)  # operands are never written
    assert torch.equal(a.detach(), z0)


def test_labels_get_no_gradient_and_other_integer_types_are_cast():
    from het_amd.layers import SoftmaxCrossEntropy, SoftmaxCrossEntropyFunction
    zd, _, lab, labd = _case(130, 9, torch.float32, 41, bad=False)
    a = zd.clone().requires_grad_(True)
    loss, stats = SoftmaxCrossEntropyFunction.apply(a, labd, -100, "mean")
    grads = torch.autograd.grad(loss, [a], allow_unused=True)
    assert grads[0] is not None and not stats.requires_grad
    mod = SoftmaxCrossEntropy()
    assert torch.equal(mod(zd, labd.to(torch.int32)), mod(zd, labd))
    with pytest.raises(ValueError, match="label"):
        SoftmaxCrossEntropy(check_labels=True)(zd, torch.where(labd == 3, torch.full_like(labd, 9), labd))
    assert float(SoftmaxCrossEntropy(check_labels=True)(zd, labd)) > 0


# --------------------------------------------------------------------------------------------------------- uninitialised buffers
@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_no_result_depends_on_uninitialised_memory(dtype, value):
    from het_amd.layers import SoftmaxCrossEntropy

    def run(N, C, seed):
        zd, _, _, labd = _case(N, C, dtype, seed)
        a = zd.clone().requires_grad_(True)
        mod = SoftmaxCrossEntropy()
        loss = mod(a, labd)
        loss.backward()
        _, lse, _ = _k().softmax_xent(zd, labd)
        return loss.detach().view(torch.int32).clone(), mod.last_stats.clone(), a.grad.clone(), lse.clone()

    for N, C, seed in ((1029, 8, 51), (130, 349, 52), (77, 3, 53)):
        clean = run(N, C, seed)
        with poisoned(value) as record:
            dirty = run(N, C, seed)
        assert record.from_module("het_amd.kernels", "_softmax_xent") and record.from_module("het_amd.kernels", "_softmax_xent_backward")
        assert record.from_module("het_amd.kernels", "_workspace")  # the partials
        for name, x, y in zip(("loss", "stats", "grad", "lse"), clean, dirty):
            assert torch.equal(x, y), f"{name} at N={N} C={C} depends on what an unwritten slot held"


# ------------------------------------------------------------------------------------- what the kernels do not take, on the device
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_strided_and_misaligned_logits_take_the_torch_composition(dtype):
    from het_amd._lib import HetError
    from het_amd.layers import SoftmaxCrossEntropy
    k = _k()
    N, C = 203, 12
    wide, _, lab, labd = _case(N, C + 4, dtype, 61)
    lab = np.where(lab >= C, -100, lab)  # (labels drawn for the wider tensor)
    lab[0], lab[1], lab[N - 1] = C, 0, -1
    labd = torch.tensor(lab, device=DEV)
    sliced = wide[:, 2:2 + C]  # a column slice of a wider tensor
    flat = torch.zeros(N * C + 8, dtype=dtype, device=DEV)
    shift = 4 // flat.element_size()
    shifted = flat[shift:shift + N * C].view(N, C)  # the base pointer 4 bytes off a 16-byte (bf16: 8-byte) boundary
    shifted.copy_(sliced)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and not sliced.is_contiguous()
    z64 = sliced.double().cpu().numpy()
    want_loss, want_lse, want_stats, _ = ref.forward(z64, lab)
    want_grad = ref.backward(z64, lab, want_lse, 1.0)
    for t in (sliced, shifted):
        assert not k.softmax_xent_ok(t, labd)
        with pytest.raises(HetError):
            k.softmax_xent(t, labd)
        with pytest.raises(HetError):
            k.softmax_xent_backward(t, labd, torch.zeros(N, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV), torch.ones((), device=DEV))
        leaf = wide.clone().requires_grad_(True) if t is sliced else flat.clone().requires_grad_(True)
        view = leaf[:, 2:2 + C] if t is sliced else leaf[shift:shift + N * C].view(N, C)
        mod = SoftmaxCrossEntropy()
        loss = mod(view, labd)
        loss.backward()
        assert_close(loss, torch.tensor(want_loss), what="fallback loss")
        assert mod.last_stats.tolist() == want_stats.tolist()
        got = leaf.grad[:, 2:2 + C] if t is sliced else leaf.grad[shift:shift + N * C].view(N, C)
        if dtype == torch.float32:
            assert_close(got, torch.tensor(want_grad), what="fallback grad")
        else:
            _assert_bf16_close(got, want_grad, "fallback grad")


# --------------------------------------------------------------------------------------- agreement with the default expression
def test_agrees_with_the_training_scripts_default_expression():
    from het_amd.layers import SoftmaxCrossEntropy
    zd, _, _, labd = _case(2049, 8, torch.float32, 71, ignored=0.0, bad=False)
    a, b = zd.clone().requires_grad_(True), zd.clone().requires_grad_(True)
    want = -b.log_softmax(dim=-1).gather(1, labd.view(-1, 1)).mean()
    want.backward()
    mod = SoftmaxCrossEntropy()
    loss = mod(a, labd)
    loss.backward()
    assert_close(loss, want.detach().cpu(), what="loss")
    # the gradient's natural size is 1 / N: compared at the size of the logits' own gradient (times N), as the expression gives it
    assert_close(a.grad * 2049, b.grad.detach().cpu() * 2049, what="grad")
    assert mod.last_stats.tolist() == [2049, int((zd.argmax(dim=1) == labd).sum()), 0]


def test_rows_past_two_to_the_31_elements():
    """N * C just above 2^31 (bf16, C = 8, all logits equal, so the expected values are known without a reference of that size):
    every index is 64-bit.  The last rows are checked: a 32-bit element offset would have wrapped onto the first ones."""
    k = _k()
    C = 8
    N = 2 ** 31 // C + 1000
    z = torch.zeros(N, C, dtype=torch.bfloat16, device=DEV)
    z[-1000:] = 1.0
    labd = torch.zeros(N, dtype=torch.int64, device=DEV)
    labd[-1000:] = 3
    labd[-500:] = -100
    loss, lse, stats = k.softmax_xent(z, labd, -100, "sum")
    assert stats.tolist() == [N - 500, N - 1000, 0]
    assert float(loss) == pytest.approx((N - 500) * np.log(8.0), rel=1e-6)
    assert float(lse[-501]) == pytest.approx(1.0 + np.log(8.0), rel=1e-6) and float(lse[-1]) == 0.0
    grad = k.softmax_xent_backward(z, labd, lse, stats, torch.tensor(8.0, device=DEV), -100, "sum")
    assert grad[-1000:-500].float().cpu().tolist() == [[1.0, 1.0, 1.0, -7.0, 1.0, 1.0, 1.0, 1.0]] * 500
    assert not bool(grad[-500:].float().any()) and grad[0].float().cpu().tolist() == [-7.0] + [1.0] * 7
