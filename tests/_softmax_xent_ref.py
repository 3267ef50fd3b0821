"""The softmax cross-entropy rule of include/het_amd.h (csrc/softmax_xent.hip, het_amd/layers.py SoftmaxCrossEntropy) in numpy
fp64: loss, lse, stats and gradient, plus the bf16 store.  Nothing here is imported from the package under test."""
import numpy as np


def rows(labels, C, ignore_index=-100):
    """(valid, bad) [N] bool: a row is valid when its label is not ignore_index and lies in [0, C); bad when it is neither."""
    labels = np.asarray(labels, dtype=np.int64)
    valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
    return valid, (labels != ignore_index) & ~valid


def argmax_first(z):
    """Lowest index among the maxima of every row, a NaN ordered above everything (torch.argmax on the CPU): the first NaN of a row
    that holds one, else the first occurrence of the row's maximum (numpy's argmax returns the first)."""
    z = np.asarray(z, dtype=np.float64)
    if z.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    nan = np.isnan(z)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, z).argmax(axis=1)).astype(np.int64)


def forward(z, labels, ignore_index=-100, reduction="mean"):
    """(loss fp64 scalar, lse [N] fp64 with 0 at skipped rows, stats int64 [3] = valid, correct, bad, row_loss [N])."""
    z = np.asarray(z, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    N, C = z.shape
    valid, bad = rows(labels, C, ignore_index)
    lab = np.where(valid, labels, 0)
    with np.errstate(all="ignore"):
        m = z.max(axis=1) if N else np.zeros(0)
        lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
        row_loss = np.where(valid, lse - z[np.arange(N), lab], 0.0)
        total = row_loss.sum()
        n_valid = int(valid.sum())
        loss = total / n_valid if reduction == "mean" and n_valid else (np.float64("nan") if reduction == "mean" else total)
    correct = int((valid & (argmax_first(z) == labels)).sum())
    return np.float64(loss), np.where(valid, lse, 0.0), np.array([n_valid, correct, int(bad.sum())], dtype=np.int64), row_loss


def backward(z, labels, lse, g=1.0, ignore_index=-100, reduction="mean"):
    """grad [N, C] fp64 = (exp(z - lse) - onehot) * g * (1 | 1 / valid); 0 in skipped rows.  ``lse``: the forward's (or the kernel's)."""
    z = np.asarray(z, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    N, C = z.shape
    valid, _ = rows(labels, C, ignore_index)
    lab = np.where(valid, labels, 0)
    scale = float(g) / max(int(valid.sum()), 1) if reduction == "mean" else float(g)
    with np.errstate(all="ignore"):
        p = np.exp(z - np.asarray(lse, dtype=np.float64)[:, None])
        p[np.arange(N), lab] -= 1.0
        return np.where(valid[:, None], p * scale, 0.0)


def to_bf16(x):
    """fp64 / fp32 values rounded once to bf16 (nearest, ties to even; a NaN stays a NaN), returned as float32."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).copy()
    out[np.isnan(f)] = np.nan
    return out.reshape(f.shape)


def float_class(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN -- elementwise."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 3, np.where(x == np.inf, 1, np.where(x == -np.inf, 2, 0)))


def draw_labels(rng, N, C, ignored=0.25, bad=True, ignore_index=-100):
    """Labels [N] int64: ~`ignored` of the rows ignore_index, and (``bad``) a few labels outside [0, C) -- C, C + 7, -1, 2^40 -- at
    random rows, the first and the last row included when there is room."""
    lab = rng.integers(0, C, size=N).astype(np.int64)
    if ignored and N:
        lab[rng.random(N) < ignored] = ignore_index
    if bad and N:
        vals = [v for v in (C, C + 7, -1, 2 ** 40) if v != ignore_index]
        pos = [0, N - 1] + list(rng.integers(0, N, size=2))
        for p, v in zip(pos, vals):
            lab[p] = v
    return lab


SPECIAL_ROWS = (  # (logits row, label): C = 4
    ([0.5, -np.inf, 1.0, -2.0], 0),        # -inf off the label: probability 0
    ([0.5, -np.inf, 1.0, -2.0], 1),        # -inf at the label: loss +inf
    ([-np.inf] * 4, 2),                    # a row of -inf: NaN
    ([0.5, np.nan, 1.0, -2.0], 0),         # a NaN off the label
    ([0.5, np.nan, 1.0, -2.0], 1),         # a NaN at the label
    ([1e4, 0.0, -1e4, 3.0], 0),            # no overflow
    ([1.0, 2.0, 3.0, 4.0], 3),             # an ordinary row among them
)
