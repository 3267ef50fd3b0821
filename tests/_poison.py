"""Control over the memory the library allocates for itself: `poisoned(value)` fills every floating-point tensor that code of the
named modules takes uninitialised (torch.empty, torch.empty_like, torch.empty_strided, Tensor.new_empty) with `value` before
the caller sees it.  A result that still matches its oracle under a poison does not depend on what an unwritten slot held; in a
test process such a slot is otherwise zeros or the recycled answer of the previous case, which passes every tolerance.

Two poisons: NaN (anything that reads it, 0 * it included, becomes NaN) and 1e30 (fmaxf(NaN, x) is x: a running-maximum slot
swallows a NaN and only a large finite value shows that it was read).  Integer tensors are never touched: a poisoned index
would be an out-of-range address.  A finite poison is clamped to the range of the tensor's type (1e30 does not fit fp16).
The patch is process-wide, not thread-local: autograd runs the backward on its own thread."""
import collections
import contextlib
import math
import sys

import torch

POISONS = (float("nan"), 1e30)
POISON_IDS = ("nan", "1e30")
_MISSING = object()


Poisoned = collections.namedtuple("Poisoned", "module function shape dtype")  # who asked for the tensor, and what it is


class Record(list):
    """What a `poisoned` block filled: one Poisoned(calling module, calling function, shape, dtype) per tensor, in allocation order."""

    def modules(self):
        return {e.module for e in self}

    def from_module(self, name, function=None):
        return [e for e in self if e.module == name and function in (None, e.function)]


def _wrap(orig, value, modules, device_type, record):
    def wrapper(*args, **kwargs):
        t = orig(*args, **kwargs)
        if isinstance(t, torch.Tensor) and t.is_floating_point() and t.numel() > 0 and t.device.type == device_type:
            frame = sys._getframe(1)
            caller = frame.f_globals.get("__name__", "")
            if caller.startswith(modules):
                top = torch.finfo(t.dtype).max  # (1e30 does not fit fp16: the largest value that does)
                with torch.no_grad():
                    t.fill_(value if math.isnan(value) else max(-top, min(top, value)))
                record.append(Poisoned(caller, frame.f_code.co_name, tuple(t.shape), t.dtype))
        return t

    wrapper.__wrapped__ = orig
    return wrapper


@contextlib.contextmanager
def poisoned(value, modules=("het_amd",), device_type="cuda"):
    """Fill what `modules` allocate uninitialised on `device_type` with `value` for the length of the block; yields the Record."""
    modules = (modules,) if isinstance(modules, str) else tuple(modules)
    record = Record()
    targets = [(torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")]
    saved = []
    try:
        for owner, name in targets:
            saved.append((owner, name, vars(owner).get(name, _MISSING)))  # (new_empty is inherited: nothing of its own to put back)
            setattr(owner, name, _wrap(getattr(owner, name), value, modules, device_type, record))
        yield record
    finally:
        for owner, name, own in reversed(saved):
            if own is _MISSING:
                delattr(owner, name)
            else:
                setattr(owner, name, own)
