"""fp64 numpy reference of the RGCN layer with block-diagonal relation weights (DGL's RelGraphConv(regularizer="bdd")), written from
the formula alone:

    out[v, b*so + j] = bias[b*so + j] + SUM_r SUM_{e: rel r, dst v} norm[eid_e] * SUM_i x[src_e, b*si + i] * weight[r, b, i, j]

and its gradients for x, weight and bias (none for norm).  The graph is a COO list (src, dst, rel, eid by position), the norm is
indexed by edge id, the blocks are weight [R, B, si, so].  Also the inputs on integer grids the GPU tests use, and the bound that
makes any fp32 summation order exact on them."""
import numpy as np


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def _i64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.int64)


def bdd_forward(num_nodes, src, dst, rel, eid, norm, x, weight, bias=None):
    """out [num_nodes, B*so] in fp64."""
    src, dst, rel, eid = _i64(src), _i64(dst), _i64(rel), _i64(eid)
    norm, x, w = _f64(norm).reshape(-1), _f64(x), _f64(weight)
    R, B, si, so = w.shape
    out = np.zeros((num_nodes, B, so))
    for r in np.unique(rel):
        e = np.nonzero(rel == r)[0]
        m = (norm[eid[e], None] * x[src[e]]).reshape(-1, B, si)
        np.add.at(out, dst[e], np.einsum("ebi,bij->ebj", m, w[r]))
    out = out.reshape(num_nodes, B * so)
    return out if bias is None else out + _f64(bias)[None, :]


def bdd_backward(num_nodes, src, dst, rel, eid, norm, x, weight, gradout):
    """(grad_x [N, B*si], grad_weight [R, B, si, so], grad_bias [B*so]) in fp64 (num_nodes: rows of x)."""
    src, dst, rel, eid = _i64(src), _i64(dst), _i64(rel), _i64(eid)
    norm, x, w, go = _f64(norm).reshape(-1), _f64(x), _f64(weight), _f64(gradout)
    R, B, si, so = w.shape
    gx = np.zeros((num_nodes, B, si))
    gw = np.zeros_like(w)
    for r in np.unique(rel):
        e = np.nonzero(rel == r)[0]
        g = (norm[eid[e], None] * go[dst[e]]).reshape(-1, B, so)
        np.add.at(gx, src[e], np.einsum("ebj,bij->ebi", g, w[r]))
        gw[r] = np.einsum("ebi,ebj->bij", x[src[e]].reshape(-1, B, si), g)
    return gx.reshape(num_nodes, B * si), gw, go.sum(0)


# ---- inputs on integer grids -------------------------------------------------------------------------------------------------
X_GRID = (-2.0, -1.0, 0.0, 1.0, 2.0)          # x and gradout
W_GRID = (-1.0, -0.5, 0.0, 0.5, 1.0)          # weight
NORM_GRID = (0.5, 1.0, 2.0)                   # norm
BIAS_GRID = tuple(i / 4 for i in range(-8, 9))
UNIT = 0.25                                   # every product norm * x * weight, and the bias, is a multiple of it


def grid_case(num_nodes, num_edges, R, K, D, B, seed, zero_rows=0.15, bias=True):
    """{"x" [N,K], "go" [N,D], "weight" [R,B,K/B,D/B], "norm" [E,1], "bias" [D] or None} as float32 numpy arrays drawn from the grids
    above, a fraction ``zero_rows`` of the rows of x and of go all zero."""
    rng = np.random.default_rng(seed)
    pick = lambda grid, shape: np.asarray(grid, dtype=np.float32)[rng.integers(0, len(grid), shape)]  # noqa: E731
    x, go = pick(X_GRID, (num_nodes, K)), pick(X_GRID, (num_nodes, D))
    x[rng.random(num_nodes) < zero_rows] = 0.0
    go[rng.random(num_nodes) < zero_rows] = 0.0
    return {"x": x, "go": go, "weight": pick(W_GRID, (R, B, K // B, D // B)), "norm": pick(NORM_GRID, (num_edges, 1)),
            "bias": pick(BIAS_GRID, (D,)) if bias else None}


def grid_units_bound(num_nodes, src, dst, rel, eid, c):
    """The largest magnitude, in units of UNIT, that any partial sum of the layer's forward or backward can reach on the grid case
    ``c``, whatever the order of the additions: the same formulas on absolute values (a partial sum of terms is bounded by the sum
    of their magnitudes), for the output, the three gradients and the (relation, node) sums ssum / gsum kept in between."""
    a = {k: (None if v is None else np.abs(v)) for k, v in c.items()}
    out = bdd_forward(num_nodes, src, dst, rel, eid, a["norm"], a["x"], a["weight"], a["bias"])
    gx, gw, gb = bdd_backward(num_nodes, src, dst, rel, eid, a["norm"], a["x"], a["weight"], a["go"])
    src, dst, eid = _i64(src), _i64(dst), _i64(eid)
    n = _f64(a["norm"]).reshape(-1)[eid, None]
    ssum = np.zeros((num_nodes, a["x"].shape[1]))
    np.add.at(ssum, dst, n * _f64(a["x"])[src])       # (all relations of a node together: at least the per-relation sums)
    gsum = np.zeros((num_nodes, a["go"].shape[1]))
    np.add.at(gsum, src, n * _f64(a["go"])[dst])
    return max(float(t.max()) for t in (out, gx, gw, gb, ssum, gsum) if t.size) / UNIT


def on_grid(t):
    """Whether every element is a whole number of UNITs."""
    v = _f64(t) / UNIT
    return bool(np.all(v == np.round(v)))
