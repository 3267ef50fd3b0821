"""The keyed dropout rule (include/het_amd.h, het_amd/layers.py KeyedDropout) in numpy, on top of het_amd.sampling.keyed_keys: the
reference of tests/test_keyed_dropout_ref.py (the torch fallback), tests/test_keyed_dropout_abi.py (T and scale) and
tests/test_gpu_keyed_dropout.py (the kernels).  Needs no GPU.

    T      = min(round-half-away(p * 65536), 65535)     scale = float32(65536 / (65536 - T))
    key(g) = keyed_keys(seed, draw, g),  g = (base + i) // 4        field = (key >> 16 * ((base + i) % 4)) & 0xFFFF
    kept = field >= T        out = a(y) * scale if kept else +0        grad_y = grad_out * scale if kept and (none or out > 0) else +0

Tensors go in and out as torch tensors (float32 or bfloat16); the arithmetic is numpy float32: one multiply, correctly rounded; a
bf16 result is rounded once, to nearest even (torch's conversion, as tests/_bf16_rows_ref.bf16_round)."""
import functools
import math

import numpy as np
import torch

from het_amd.sampling import keyed_keys

SPECIALS = (-0.0, 0.0, 1e-40, -1e-40, float("inf"), float("-inf"), float("nan"))  # (1e-40: an fp32 denormal; bf16 rounds it to one of its own)
RATES = (0.0, 2.0 ** -16, 0.1, 1.0 / 3.0, 0.5, 0.9, 65535.0 / 65536.0)


def params(p):
    """(T, scale as np.float32) of a rate p in [0, 1)."""
    assert 0.0 <= p < 1.0
    x = p * 65536.0
    T = int(math.floor(x))
    if x - T >= 0.5:  # (x - floor(x) is exact)
        T += 1
    T = min(T, 65535)
    return T, np.float32(65536.0 / (65536 - T))


@functools.lru_cache(maxsize=8)
def fields(seed, draw, base, n):
    """The 16-bit field of each of n elements from `base` on: numpy uint64 [n] (cached: the tests share it; never written)."""
    assert base >= 0 and base % 4 == 0
    groups = np.uint64(base // 4) + np.arange((n + 3) // 4, dtype=np.uint64)
    key = keyed_keys(seed, draw, groups)
    f = np.stack([(key >> np.uint64(16 * j)) & np.uint64(0xFFFF) for j in range(4)], axis=1).reshape(-1)[:n]
    f.setflags(write=False)
    return f


def mask(seed, draw, base, n, p):
    """kept [n]: numpy bool."""
    return fields(seed, draw, base, n) >= np.uint64(params(p)[0])


def _f32(t):
    return t.detach().cpu().to(torch.float32).contiguous().view(-1).numpy()


def forward(y, p, seed, draw, relu=False, base=0):
    """out of the rule for a float32 / bfloat16 tensor y (any device; the result is a CPU tensor of y's dtype and shape)."""
    _, scale = params(p)
    v = _f32(y)
    if relu:
        v = np.where(v < 0, np.float32(0), v)
    with np.errstate(all="ignore"):
        out = np.where(mask(seed, draw, base, v.size, p), v * scale, np.float32(0)).astype(np.float32)
    return torch.from_numpy(out).view(y.shape).to(y.dtype)


def backward(grad_out, out, p, seed, draw, relu=False, base=0):
    """grad_y of the rule; `out` is the forward's result (read for relu only)."""
    _, scale = params(p)
    g = _f32(grad_out)
    kept = mask(seed, draw, base, g.size, p)
    if relu:
        kept = kept & (_f32(out) > 0)
    with np.errstate(all="ignore"):
        gy = np.where(kept, g * scale, np.float32(0)).astype(np.float32)
    return torch.from_numpy(gy).view(grad_out.shape).to(grad_out.dtype)


def special_input(n, dtype, seed):
    """n values in `dtype` drawn from N(0, 1) (rounded once for bf16), with every value of SPECIALS written at up to 6 places each,
    spread over the tensor -- so that at p = 0.5 each lands on kept and on dropped positions (asserted in test_keyed_dropout_ref)."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(n, generator=gen)
    k = len(SPECIALS)
    stride = max(1, n // (6 * k))
    for rep in range(6 if n >= 6 * k else 1):  # (a tensor too short for all of them keeps some ordinary values)
        for j, s in enumerate(SPECIALS):
            at = (rep * k + j) * stride + (rep % 4 if stride >= 8 else 0)  # (every place in a group of 4 gets its turn)
            if at < n:
                y[at] = s
    return y.to(dtype)


def same_bits(a, b, what=""):
    """torch.equal on the bit patterns, with a NaN equal to a NaN (torch.equal itself holds no NaN equal to anything, and the sign
    and payload a NaN leaves a conversion with are not part of the rule): same dtype, same shape, NaNs at the same places, and the
    same bits -- so +0 is not -0 -- everywhere else."""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaNs at different places ({int(na.sum())} vs {int(nb.sum())})"
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    ia, ib = a.contiguous().view(bits).masked_fill(na, 0), b.contiguous().view(bits).masked_fill(nb, 0)
    if not torch.equal(ia, ib):
        bad = (ia != ib).view(-1).nonzero().view(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} elements differ; first at {i}: {a.view(-1)[i].item()!r} vs {b.view(-1)[i].item()!r}")
