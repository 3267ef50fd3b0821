"""The numpy reference of the softmax cross-entropy rule (tests/_softmax_xent_ref.py) held against torch on the CPU in fp64, and the
module's torch composition (het_amd/layers.py SoftmaxCrossEntropy on CPU tensors) held against the reference.  Runs without a GPU;
fails on a tree without the feature."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _softmax_xent_ref as ref

SHAPES = ((1, 1), (5, 1), (7, 3), (64, 8), (33, 17), (9, 349))


def _case(N, C, seed, ignored=0.25, ignore_index=-100):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, C)) * 3.0
    lab = ref.draw_labels(rng, N, C, ignored=ignored, bad=False, ignore_index=ignore_index)
    if ignored and N >= 2:
        lab[0], lab[1] = ignore_index, (1 if ignore_index == 0 else 0) % C if C > 1 else 0
    return z, lab


def _torch_ce(z, lab, ignore_index, reduction):
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    loss = F.cross_entropy(zt, torch.tensor(lab), ignore_index=ignore_index, reduction=reduction)
    if loss.requires_grad and bool(torch.isfinite(loss)):
        loss.backward()
    return loss.detach().numpy(), (zt.grad.numpy() if zt.grad is not None else np.zeros_like(z))


@pytest.mark.parametrize("reduction", ("mean", "sum"))
@pytest.mark.parametrize("ignored", (0.0, 0.25))
@pytest.mark.parametrize("N,C", SHAPES)
def test_reference_is_torch_cross_entropy_in_fp64(N, C, ignored, reduction):
    ignore_index = -100
    z, lab = _case(N, C, 11 * N + C, ignored, ignore_index)
    valid, bad = ref.rows(lab, C, ignore_index)
    if ignored and N >= 2 and C > 1:
        assert (~valid).any() and valid.any()  # at least one ignored and one valid row
    assert not bad.any()
    loss, lse, stats, _ = ref.forward(z, lab, ignore_index, reduction)
    want, want_grad = _torch_ce(z, lab, ignore_index, reduction)
    np.testing.assert_allclose(loss, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.backward(z, lab, lse, 1.0, ignore_index, reduction), want_grad, rtol=1e-11, atol=1e-14)
    am = torch.argmax(torch.tensor(z), dim=1).numpy()
    assert stats.tolist() == [int(valid.sum()), int((valid & (am == lab)).sum()), 0]
    np.testing.assert_array_equal(lse[~valid], 0.0)
    np.testing.assert_allclose(lse[valid], torch.logsumexp(torch.tensor(z), dim=1).numpy()[valid], rtol=1e-13)


def test_ignore_index_that_is_a_class_number():
    z, lab = _case(40, 5, 3, ignored=0.3, ignore_index=2)
    valid, bad = ref.rows(lab, 5, 2)
    assert (~valid).any() and valid.any() and not bad.any() and (lab == 2).any()
    for reduction in ("mean", "sum"):
        loss, lse, stats, _ = ref.forward(z, lab, 2, reduction)
        want, want_grad = _torch_ce(z, lab, 2, reduction)
        np.testing.assert_allclose(loss, want, rtol=1e-12)
        np.testing.assert_allclose(ref.backward(z, lab, lse, 1.0, 2, reduction), want_grad, rtol=1e-11, atol=1e-14)
        assert stats[0] == int((lab != 2).sum()) and stats[2] == 0


def test_no_rows_and_no_valid_rows():
    for z, lab in ((np.zeros((0, 4)), np.zeros(0, dtype=np.int64)), (np.ones((3, 4)), np.full(3, -100))):
        loss, lse, stats, _ = ref.forward(z, lab, -100, "mean")
        assert np.isnan(loss) and stats.tolist() == [0, 0, 0] and lse.shape == (z.shape[0],)
        assert np.isnan(_torch_ce(z, lab, -100, "mean")[0])  # torch's mean over no rows
        assert ref.forward(z, lab, -100, "sum")[0] == 0.0
        g = ref.backward(z, lab, lse, 1.0, -100, "mean")
        assert g.shape == z.shape and not g.any() and not np.signbit(g).any()


def test_specials_match_torch_by_class():
    z = np.array([r for r, _ in ref.SPECIAL_ROWS], dtype=np.float64)
    lab = np.array([l for _, l in ref.SPECIAL_ROWS], dtype=np.int64)
    _, lse, _, row_loss = ref.forward(z, lab, -100, "sum")
    zt = torch.tensor(z, dtype=torch.float32, requires_grad=True)
    want = F.cross_entropy(zt, torch.tensor(lab), reduction="none")
    want.sum().backward()
    np.testing.assert_array_equal(ref.float_class(row_loss), ref.float_class(want.detach().numpy()))
    np.testing.assert_array_equal(ref.float_class(ref.backward(z, lab, lse, 1.0, -100, "sum")), ref.float_class(zt.grad.numpy()))
    assert ref.float_class(row_loss).tolist() == [0, 1, 3, 3, 3, 0, 0]
    assert row_loss[5] == 0.0  # one logit 1e4 above the rest: no overflow, loss 0


def test_argmax_ties_resolve_to_the_lowest_index_and_nan_is_the_maximum():
    rng = np.random.default_rng(5)
    z = rng.integers(-2, 3, size=(200, 6)).astype(np.float64)  # a small integer grid: exact ties in most rows
    assert (np.sort(z, axis=1)[:, -1] == np.sort(z, axis=1)[:, -2]).sum() > 50
    z[3, 4] = np.nan
    z[4, [1, 5]] = np.nan
    np.testing.assert_array_equal(ref.argmax_first(z), torch.argmax(torch.tensor(z), dim=1).numpy())
    assert ref.argmax_first(z)[3] == 4 and ref.argmax_first(z)[4] == 1


def test_bf16_store_emulation_is_torch_rounding():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-8, 8, 4096), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.00390625, 1.01171875]])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(ref.to_bf16(x).view(np.uint32)[~np.isnan(x)], want.view(np.uint32)[~np.isnan(x)])
    assert np.isnan(ref.to_bf16(x)[np.isnan(x)]).all()


# ---- the module on CPU tensors: the torch composition of the same rule
def _module_case(N, C, seed, dtype=torch.float32, ignore_index=-100, bad=True):
    rng = np.random.default_rng(seed)
    z = torch.tensor(rng.standard_normal((N, C)) * 2.0).to(dtype)
    lab = ref.draw_labels(rng, N, C, ignored=0.25, bad=bad, ignore_index=ignore_index)
    if N >= 4:
        lab[1], lab[2] = ignore_index, (ignore_index + 1) % C
    return z, lab


@pytest.mark.parametrize("reduction", ("mean", "sum"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64, torch.float16, torch.bfloat16))
@pytest.mark.parametrize("N,C", ((1, 1), (37, 3), (64, 8), (20, 349), (0, 5)))
def test_module_cpu_fallback(N, C, dtype, reduction):
    from het_amd.layers import SoftmaxCrossEntropy
    z, lab = _module_case(N, C, 7 * N + C, dtype)
    valid, bad = ref.rows(lab, C)
    if N >= 4:
        assert (~valid).any() and bad.any() and (valid.any() or C == 1)
    zg = z.clone().requires_grad_(True)
    labels = torch.tensor(lab)
    mod = SoftmaxCrossEntropy(reduction=reduction)
    loss = mod(zg, labels)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward(torch.tensor(-2.5))
    want_loss, lse, stats, _ = ref.forward(z.double().numpy(), lab, -100, reduction)
    want_grad = ref.backward(z.double().numpy(), lab, lse, -2.5, -100, reduction)
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    np.testing.assert_allclose(loss.detach().double().numpy(), want_loss, rtol=tol, atol=tol, equal_nan=True)
    gtol = {torch.float64: 1e-12, torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dtype]
    np.testing.assert_allclose(zg.grad.double().numpy(), want_grad, rtol=gtol, atol=gtol * max(1.0, float(np.abs(want_grad).max(initial=0.0))))
    assert zg.grad.dtype == dtype and torch.equal(zg.detach(), z)
    assert mod.last_stats.dtype == torch.int64 and mod.last_stats.tolist() == stats.tolist()
    acc = mod.accuracy()
    if stats[0]:
        assert float(acc) == pytest.approx(stats[1] / stats[0])
    else:
        assert bool(torch.isnan(acc))
    if N:  # bad labels contribute nothing: the same loss and gradient with those rows ignored
        lab2 = np.where(bad, -100, lab)
        z2 = z.clone().requires_grad_(True)
        loss2 = SoftmaxCrossEntropy(reduction=reduction)(z2, torch.tensor(lab2))
        loss2.backward(torch.tensor(-2.5))
        assert torch.equal(loss2.detach(), loss.detach()) or (torch.isnan(loss2) and torch.isnan(loss))
        assert torch.equal(z2.grad, zg.grad)
        assert not zg.grad[torch.tensor(~valid)].any()


def test_module_labels_of_another_integer_type_and_custom_ignore_index():
    from het_amd.layers import SoftmaxCrossEntropy
    z, lab = _module_case(50, 6, 2, ignore_index=3, bad=False)
    valid, bad = ref.rows(lab, 6, 3)
    assert (~valid).any() and valid.any() and not bad.any()
    mod = SoftmaxCrossEntropy(ignore_index=3)
    a = mod(z, torch.tensor(lab))
    b = mod(z, torch.tensor(lab, dtype=torch.int32))
    assert torch.equal(a, b)
    want = F.cross_entropy(z, torch.tensor(lab), ignore_index=3)
    torch.testing.assert_close(a, want, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        mod(z, torch.tensor(lab).float())
    with pytest.raises(ValueError):
        SoftmaxCrossEntropy(reduction="none")


def test_check_labels_raises_on_a_bad_label():
    from het_amd.layers import SoftmaxCrossEntropy
    z = torch.zeros(6, 4)
    for badv in (4, -1):
        lab = torch.tensor([0, 1, badv, 3, -100, 2])
        with pytest.raises(ValueError, match="1 label"):
            SoftmaxCrossEntropy(check_labels=True)(z, lab)
        quiet = SoftmaxCrossEntropy()
        loss = quiet(z, lab)
        assert quiet.last_stats.tolist() == [4, 1, 1]  # (all logits equal: only label 0 is the first maximum)
        torch.testing.assert_close(loss, torch.tensor(float(np.log(4.0)), dtype=torch.float32))
    assert float(SoftmaxCrossEntropy(check_labels=True)(z, torch.tensor([0, 1, -100, 3, -100, 2]))) > 0


def test_module_specials_match_torch_by_class_on_the_cpu():
    from het_amd.layers import SoftmaxCrossEntropy
    z = torch.tensor([r for r, _ in ref.SPECIAL_ROWS], dtype=torch.float32)
    lab = torch.tensor([l for _, l in ref.SPECIAL_ROWS])
    for i in range(z.shape[0]):
        zi, zt = z[i:i + 1].clone().requires_grad_(True), z[i:i + 1].clone().requires_grad_(True)
        loss = SoftmaxCrossEntropy(reduction="sum")(zi, lab[i:i + 1])
        want = F.cross_entropy(zt, lab[i:i + 1], reduction="sum")
        loss.backward()
        want.backward()
        assert ref.float_class(loss.detach().numpy()) == ref.float_class(want.detach().numpy()), i
        np.testing.assert_array_equal(ref.float_class(zi.grad.numpy()), ref.float_class(zt.grad.numpy()), err_msg=str(i))


def test_module_autograd_contract_on_the_cpu():
    from het_amd.layers import SoftmaxCrossEntropy, SoftmaxCrossEntropyFunction
    z, lab = _module_case(30, 5, 9)
    labels = torch.tensor(lab)
    mod = SoftmaxCrossEntropy()
    assert not mod(z, labels).requires_grad  # the logits need no gradient
    zg = z.clone().requires_grad_(True)
    train = mod(zg, labels)
    with torch.no_grad():
        a = mod(zg, labels)
    with torch.inference_mode():
        b = mod(zg, labels)
    assert torch.equal(a, train.detach()) and torch.equal(b.clone(), train.detach()) and not a.requires_grad
    train.backward(retain_graph=True)
    g1 = zg.grad.clone()
    train.backward()
    assert torch.equal(zg.grad, 2 * g1)  # .grad accumulates; the second backward gave the same bits
    loss, stats = SoftmaxCrossEntropyFunction.apply(zg, labels, -100, "mean")
    assert not stats.requires_grad and loss.requires_grad
    zd = z.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: SoftmaxCrossEntropy(reduction="sum")(t, labels), (zd,))
