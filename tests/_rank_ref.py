"""The rule of filtered DistMult ranking (het_amd/linkpred.py, include/het_amd.h) restated in numpy, scores in fp64:

    query j    (a_j, r_j, t_j): anchor, relation, true node.  Tail ranking of (s, r, o): a = s, t = o; head ranking: a = o, t = s;
               sides="both": the P tail queries, then the P head queries.
    run        [lo_j, hi_j) = the run of the offsets that holds t_j ([0, N) without offsets)
    q_j[d]     = fl32(h[a_j, d] * w[r_j, d])   (the one rounding the reference keeps: the product in float32)
    score_j(c) = sum_d q_j[d] * h[c, d], here in fp64;  p_j = score_j(t_j)
    excluded   c == t_j; for a tail query every c with (a_j, r_j, c) among the filter triples, for a head query every c with
               (c, r_j, a_j); sets: a c listed twice is excluded once; a c outside the run changes nothing
    greater / equal / cands = the number of c in the run, not excluded, with score_j(c) > p_j / == p_j / at all
    bad        a or t outside [0, N), r outside [0, R), t in no run: the three counts are 0

On integer grids every order of the sum is exact, so the fp64 counts are the fp32 chain's.  On other inputs `interval=True` gives,
with u = 2^-24 and g = (D + 1) u / (1 - (D + 1) u), tol_j(c) = g (sum_d |q_j[d] h[c, d]| + sum_d |q_j[d] h[t_j, d]|) -- the bound of
two fp32 fma chains of D terms against their exact sums -- the counts lo_j = #{score - p > tol} and hi_j = #{score - p >= -tol}: any
correct fp32 chain has lo_j <= greater_j and greater_j + equal_j <= hi_j."""
import numpy as np


def queries(s, r, o, sides):
    s, r, o = (np.asarray(x, dtype=np.int64) for x in (s, r, o))
    f = np.zeros(len(s), dtype=bool)
    if sides == "tail":
        return s, r, o, f
    if sides == "head":
        return o, r, s, ~f
    assert sides == "both"
    return np.concatenate([s, o]), np.concatenate([r, r]), np.concatenate([o, s]), np.concatenate([f, ~f])


def known_sets(filt, N, R):
    """({(s, r): {o}}, {(r, o): {s}}) of the filter triples with every id in range."""
    tails, heads = {}, {}
    if filt is not None:
        for s, r, o in zip(*(np.asarray(x, dtype=np.int64).tolist() for x in filt)):
            if 0 <= s < N and 0 <= o < N and 0 <= r < R:
                tails.setdefault((s, r), set()).add(o)
                heads.setdefault((r, o), set()).add(s)
    return tails, heads


def filter_pairs(filt, a, r, head, N, R):
    """The set of (query, excluded candidate) pairs, by a Python set construction."""
    tails, heads = known_sets(filt, N, R)
    out = set()
    for j, (aj, rj, hj) in enumerate(zip(np.asarray(a).tolist(), np.asarray(r).tolist(), np.asarray(head).tolist())):
        for c in (heads.get((rj, aj), ()) if hj else tails.get((aj, rj), ())):
            out.add((j, c))
    return out


def rank_reference(h, w, s, r, o, sides="both", filt=None, offsets=None, interval=False):
    """dict(greater, equal, cands [Q] int64, bad [Q] bool, and with `interval` lo, hi [Q] int64) of the rule above.  h [N, D] and w
    [R, D]: arrays of float32-representable values (a bf16 table: its widened values)."""
    h32, w32 = np.asarray(h, dtype=np.float32), np.asarray(w, dtype=np.float32)
    (N, D), R = h32.shape, w32.shape[0]
    a, rr, t, head = queries(s, r, o, sides)
    Q = len(a)
    tails, heads = known_sets(filt, N, R)
    offs = None if offsets is None else np.asarray(offsets, dtype=np.int64)
    h64 = h32.astype(np.float64)
    out = {k: np.zeros(Q, dtype=np.int64) for k in ("greater", "equal", "cands", "lo", "hi")}
    out["bad"] = np.zeros(Q, dtype=bool)
    g = (D + 1) * 2.0 ** -24 / (1 - (D + 1) * 2.0 ** -24)
    for j in range(Q):
        aj, rj, tj = int(a[j]), int(rr[j]), int(t[j])
        ok = 0 <= aj < N and 0 <= tj < N and 0 <= rj < R
        lo, hi = 0, N
        if ok and offs is not None:
            ok = offs[0] <= tj < offs[-1]
            if ok:
                ty = int(np.searchsorted(offs, tj, side="right")) - 1
                lo, hi = max(int(offs[ty]), 0), min(int(offs[ty + 1]), N)
        if not ok:
            out["bad"][j] = True
            continue
        q = (h32[aj] * w32[rj]).astype(np.float64)  # (the float32 product, then exact)
        sc = h64[lo:hi] @ q
        p = float(h64[tj] @ q)
        keep = np.ones(hi - lo, dtype=bool)
        keep[tj - lo] = False
        for c in (heads.get((rj, aj), ()) if head[j] else tails.get((aj, rj), ())):
            if lo <= c < hi:
                keep[c - lo] = False
        out["greater"][j] = int((keep & (sc > p)).sum())
        out["equal"][j] = int((keep & (sc == p)).sum())
        out["cands"][j] = int(keep.sum())
        if interval:
            tol = g * (np.abs(h64[lo:hi] * q).sum(1) + np.abs(h64[tj] * q).sum())
            out["lo"][j] = int((keep & (sc - p > tol)).sum())
            out["hi"][j] = int((keep & (sc - p >= -tol)).sum())
    if not interval:
        del out["lo"], out["hi"]
    return out


def integer_case(N, R, D, P, seed, bf16=False):
    """h in -2..2 and w in {-1, 0, 1, 2} (exact in bf16 too, exact sums in any order, plenty of ties), P triples."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-2, 3, size=(N, D)).astype(np.float32)
    w = rng.integers(-1, 3, size=(R, D)).astype(np.float32)
    s, r, o = rng.integers(0, N, size=P), rng.integers(0, R, size=P), rng.integers(0, N, size=P)
    return h, w, s, r, o


def normal_case(D, N, Q, seed, R=5):
    """Standard-normal h and w from default_rng(seed) and Q tail queries: the cases of the decidedness table."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((N, D)).astype(np.float32)
    w = rng.standard_normal((R, D)).astype(np.float32)
    s, r, o = rng.integers(0, N, size=Q), rng.integers(0, R, size=Q), rng.integers(0, N, size=Q)
    return h, w, s, r, o


NORMAL_CASES = ((64, 1031, 130, 0), (100, 1031, 130, 1), (256, 515, 70, 3))
