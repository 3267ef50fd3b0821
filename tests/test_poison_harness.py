"""tests/_poison.py on the CPU: what it fills, what it leaves alone, that it always goes away again, and the two defects it exists
to catch -- with the reason there are two poison values."""
import math
import threading

import pytest
import torch

from tests import _poison
from tests._poison import POISONS, poisoned

ME = __name__
FLOATS = (torch.float32, torch.bfloat16, torch.float16, torch.float64)
ENTRY_POINTS = {
    "empty": lambda dt: torch.empty(3, 5, dtype=dt),
    "empty_like": lambda dt: torch.empty_like(torch.zeros(3, 5, dtype=dt)),
    "empty_strided": lambda dt: torch.empty_strided((3, 5), (5, 1), dtype=dt),
    "new_empty": lambda dt: torch.zeros(2, dtype=dt).new_empty((3, 5)),
}
ORIGINALS = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)


def _holds(t, value):
    """Every element is `value` as the tensor's dtype holds it (1e30 does not fit fp16: its largest finite value)."""
    want = torch.full_like(t, min(value, torch.finfo(t.dtype).max))
    return bool(torch.isnan(t).all()) if math.isnan(value) else bool(torch.equal(t, want))


def _patch_is_gone():
    return (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == ORIGINALS and "new_empty" not in vars(torch.Tensor)


@pytest.mark.parametrize("value", POISONS, ids=_poison.POISON_IDS)
@pytest.mark.parametrize("dtype", FLOATS, ids=str)
@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_floats_are_filled(entry, dtype, value):
    with poisoned(value, modules=(ME,), device_type="cpu") as rec:
        t = ENTRY_POINTS[entry](dtype)
    assert t.shape == (3, 5) and t.dtype == dtype
    assert _holds(t, value)
    assert list(rec) == [(ME, "<lambda>", (3, 5), dtype)]


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_ints_and_bools_are_untouched(entry):
    for dt in (torch.int64, torch.int32, torch.uint8, torch.bool):
        with poisoned(1e30, modules=(ME,), device_type="cpu") as rec:
            t = ENTRY_POINTS[entry](dt)
            t.zero_()  # (whatever it held, nothing was written into it that would not fit)
        assert t.dtype == dt and not rec


def test_empty_tensors_are_not_recorded():
    with poisoned(1e30, modules=(ME,), device_type="cpu") as rec:
        torch.empty(0, 4)
        torch.zeros(0).new_empty((0,))
    assert not rec


def test_callers_outside_the_modules_are_untouched():
    """This module is not het_amd: with the default modules its allocations keep their bits, and so do torch's own (torch.zeros_like
    and friends allocate below this frame)."""
    with poisoned(float("nan"), device_type="cpu") as rec:
        a = torch.empty(64)
        a.zero_()
        b = torch.zeros(4).new_empty((64,)).zero_()
        c = torch.empty_like(a).zero_()
    assert not rec
    assert not torch.isnan(a).any() and not torch.isnan(b).any() and not torch.isnan(c).any()
    # module names are matched by prefix (a package covers its submodules)
    with poisoned(float("nan"), modules=(ME[:-3],), device_type="cpu") as rec:
        torch.empty(2)
    assert len(rec) == 1
    with poisoned(float("nan"), modules=("oracle",), device_type="cpu") as rec:
        torch.empty(2)
    assert not rec


def test_other_device_types_are_untouched():
    with poisoned(float("nan"), modules=(ME,), device_type="cuda") as rec:
        t = torch.empty(8)
    assert not rec and t.device.type == "cpu"


def test_the_record_names_module_function_shape_and_dtype():
    with poisoned(1e30, modules=(ME,), device_type="cpu") as rec:
        torch.empty(2, 3)
        torch.empty(7, dtype=torch.int64)
        torch.empty_like(torch.zeros(4, dtype=torch.bfloat16))
        torch.zeros(1, dtype=torch.float64).new_empty((5, 1))
    fn = "test_the_record_names_module_function_shape_and_dtype"
    assert list(rec) == [(ME, fn, (2, 3), torch.float32), (ME, fn, (4,), torch.bfloat16), (ME, fn, (5, 1), torch.float64)]
    assert rec[1].module == ME and rec[1].function == fn and rec[1].shape == (4,) and rec[1].dtype == torch.bfloat16
    assert rec.modules() == {ME} and rec.from_module(ME) == list(rec) and rec.from_module("het_amd.kernels") == []
    assert rec.from_module(ME, fn) == list(rec) and rec.from_module(ME, "_workspace") == []


def test_the_patch_is_gone_after_the_block_and_after_an_exception():
    assert _patch_is_gone()
    with poisoned(1e30, modules=(ME,), device_type="cpu"):
        assert not _patch_is_gone()
    assert _patch_is_gone()
    with pytest.raises(ZeroDivisionError):
        with poisoned(1e30, modules=(ME,), device_type="cpu"):
            1 / 0
    assert _patch_is_gone()
    t = torch.empty(16)
    t.zero_()
    assert not _holds(t, 1e30)


def test_the_patch_is_process_wide():
    """Autograd runs the backward on a worker thread: an allocation made there is poisoned too."""
    got = []
    with poisoned(1e30, modules=(ME,), device_type="cpu") as rec:
        th = threading.Thread(target=lambda: got.append(torch.empty(4)))
        th.start()
        th.join()
    assert _holds(got[0], 1e30) and len(rec) == 1


def test_nesting_restores_in_order():
    with poisoned(1e30, modules=(ME,), device_type="cpu") as outer:
        with poisoned(float("nan"), modules=(ME,), device_type="cpu") as inner:
            pass
        t = torch.empty(3)
    assert _patch_is_gone() and _holds(t, 1e30) and len(outer) == 1 and not inner


# ---------------------------------------------------------------- the defects this is for
def _sum_of_half_written(x):
    """A deliberately wrong routine: writes the first half of its scratch buffer and sums all of it."""
    buf = torch.empty(2 * x.numel())
    buf[:x.numel()] = x
    return buf.sum()


def _max_of_half_written(x):
    """The same defect under a running maximum, as fmaxf computes it (a NaN operand is dropped)."""
    buf = torch.empty(2 * x.numel())
    buf[:x.numel()] = x
    return torch.fmax(buf[:x.numel()], buf[x.numel():]).max()


@pytest.mark.parametrize("value", POISONS, ids=_poison.POISON_IDS)
def test_a_sum_over_a_half_written_buffer_is_caught_by_both_poisons(value):
    x = torch.arange(1.0, 9.0)
    with poisoned(value, modules=(ME,), device_type="cpu") as rec:
        got = _sum_of_half_written(x)
    assert rec
    assert not torch.isclose(got, x.sum())


def test_a_maximum_over_a_half_written_buffer_is_missed_by_nan_and_caught_by_1e30():
    """Why there are two values: fmax(NaN, x) = x, so the NaN-poisoned run returns the right answer; 1e30 does not."""
    x = torch.arange(1.0, 9.0)
    with poisoned(float("nan"), modules=(ME,), device_type="cpu") as rec:
        missed = _max_of_half_written(x)
    assert rec and float(missed) == float(x.max())
    with poisoned(1e30, modules=(ME,), device_type="cpu") as rec:
        caught = _max_of_half_written(x)
    assert rec and float(caught) > 1e29 > float(x.max())
