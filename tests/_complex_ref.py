"""The ComplEx rule of het_amd/linkpred.py (include/het_amd.h) restated independently in numpy: fp64 scores and
gradients, an fp32 staged emulation of the two gradient sums in the order the kernels state (csrc/triple_score.hip), and the ranking
rule with q in exact float32.  No torch, no het_amd import.

Layout: h [N, D], w [R, D], D even; column 2k is the real and column 2k + 1 the imaginary part of component k.  With a = h[s],
b = w[r], c = h[o]:

    score      = sum_k Re(a_k b_k conj(c_k)) = sum_k (a_r b_r - a_i b_i) c_r + (a_r b_i + a_i b_r) c_i
    grad a_r  += g (b_r c_r + b_i c_i)      grad a_i += g (b_r c_i - b_i c_r)      (slot side 0: the node is the head)
    grad c_r  += g (a_r b_r - a_i b_i)      grad c_i += g (a_r b_i + a_i b_r)      (slot side 1: the node is the tail)
    grad b_r  += g (a_r c_r + a_i c_i)      grad b_i += g (a_r c_i - a_i c_r)

Ranking: query (a, r, t, side); side 0 ranks tails (the anchor is the head), side 1 ranks heads (the anchor is the tail).  With
x = h[a], b = w[r], every operation a float32 one:

    side 0:  q[2k] = (x_r b_r) - (x_i b_i)     q[2k+1] = (x_r b_i) + (x_i b_r)
    side 1:  q[2k] = (b_r x_r) + (b_i x_i)     q[2k+1] = (b_r x_i) - (b_i x_r)
    score(c) = sum_d q[d] h[c, d];  p = score(t);  the run, the exclusions, the counts and the intervals are tests/_rank_ref.py's."""
import numpy as np

from tests import _rank_ref
from tests._triple_ref import good, slot_lists


def parts(x):
    return x[..., 0::2], x[..., 1::2]


def join(re, im):
    out = np.empty(re.shape[:-1] + (2 * re.shape[-1],), dtype=re.dtype)
    out[..., 0::2], out[..., 1::2] = re, im
    return out


def scores(h, w, s, r, o):
    """fp64 scores [T]; +0 for a triple with an id outside its table."""
    h, w = np.asarray(h, dtype=np.float64), np.asarray(w, dtype=np.float64)
    s, r, o = (np.asarray(x, dtype=np.int64) for x in (s, r, o))
    ok = good(s, r, o, h.shape[0], w.shape[0])
    out = np.zeros(len(s))
    (ar, ai), (br, bi), (cr, ci) = parts(h[s[ok]]), parts(w[r[ok]]), parts(h[o[ok]])
    out[ok] = ((ar * br - ai * bi) * cr + (ar * bi + ai * br) * ci).sum(-1)
    return out


def scores_by_complex_numbers(h, w, s, r, o):
    """The same scores through numpy's complex128: sum_k Re(a_k b_k conj(c_k)) -- the layout and the conjugate stated a second way."""
    z = lambda x: np.asarray(x, dtype=np.float64)[..., 0::2] + 1j * np.asarray(x, dtype=np.float64)[..., 1::2]  # noqa: E731
    s, r, o = (np.asarray(x, dtype=np.int64) for x in (s, r, o))
    return (z(h)[s] * z(w)[r] * np.conj(z(h)[o])).real.sum(-1)


def grads(h, w, s, r, o, g):
    """(grad_h [N, D], grad_w [R, D]) in fp64."""
    h, w, g = np.asarray(h, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s, r, o = (np.asarray(x, dtype=np.int64) for x in (s, r, o))
    ok = good(s, r, o, h.shape[0], w.shape[0])
    s, r, o, g = s[ok], r[ok], o[ok], g[ok][:, None]
    (ar, ai), (br, bi), (cr, ci) = parts(h[s]), parts(w[r]), parts(h[o])
    gh, gw = np.zeros_like(h), np.zeros_like(w)
    np.add.at(gh, s, join(g * (br * cr + bi * ci), g * (br * ci - bi * cr)))
    np.add.at(gh, o, join(g * (ar * br - ai * bi), g * (ar * bi + ai * br)))
    np.add.at(gw, r, join(g * (ar * cr + ai * ci), g * (ar * ci - ai * cr)))
    return gh, gw


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32 (the
    second rounding differs from a true fused one in rare halfway cases only: this emulation is a yardstick, not a bit reference)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def staged_grads(h, w, s, r, o, g, L, rel_chunk):
    """The two sums in fp32 in the kernels' stated order and arithmetic.  Per node, in ascending slot from +0, with u = fl(g b_r),
    v = fl(g b_i) (v negated on a tail slot) and x the other end: re = fma(v, x_i, fma(u, x_r, re)), im = fma(-v, x_r, fma(u, x_i, im));
    a list longer than L in chunks of L from its start, the chunk sums added in chunk order.  Per relation, in ascending j in chunks
    of ``rel_chunk``: re = fma(fma(a_i, c_i, fl(a_r c_r)), g, re), im = fma(fma(-a_i, c_r, fl(a_r c_i)), g, im); the chunk sums in
    chunk order."""
    f = np.float32
    h, w, g = np.asarray(h, dtype=f), np.asarray(w, dtype=f), np.asarray(g, dtype=f)
    s, r, o = (np.asarray(x, dtype=np.int64) for x in (s, r, o))
    N, R = h.shape[0], w.shape[0]
    half = h.shape[1] // 2
    nodes, rels = slot_lists(s, r, o, N, R)

    def node_run(slots):
        re, im = np.zeros(half, dtype=f), np.zeros(half, dtype=f)
        for e in slots:
            j, tail = e >> 1, e & 1
            br, bi = parts(w[r[j]])
            xr, xi = parts(h[s[j] if tail else o[j]])
            u, v = g[j] * br, g[j] * bi
            if tail:
                v = -v
            re = fma32(v, xi, fma32(u, xr, re))
            im = fma32(-v, xr, fma32(u, xi, im))
        return join(re, im)

    def rel_run(js):
        re, im = np.zeros(half, dtype=f), np.zeros(half, dtype=f)
        for j in js:
            (ar, ai), (cr, ci) = parts(h[s[j]]), parts(h[o[j]])
            gj = np.full(half, g[j], dtype=f)
            re = fma32(fma32(ai, ci, ar * cr), gj, re)
            im = fma32(fma32(-ai, cr, ar * ci), gj, im)
        return join(re, im)

    def chunked(items, run, size, always):
        if len(items) <= size and not always:
            return run(items)
        acc = np.zeros(h.shape[1], dtype=f)
        for c in range(0, len(items), size):
            acc = acc + run(items[c:c + size])
        return acc

    gh, gw = np.zeros_like(h), np.zeros_like(w)
    for v, slots in enumerate(nodes):
        gh[v] = chunked(slots, node_run, L, False)
    for rel, js in enumerate(rels):
        gw[rel] = chunked(js, rel_run, rel_chunk, True)
    return gh, gw


# ---- ranking ----------------------------------------------------------------------------------------------------------------------
def rank_q(x, b, side):
    """q [D] float32 of the rule for one query: x = h[a], b = w[r] float32 rows; three float32 roundings per element."""
    x, b = np.asarray(x, dtype=np.float32), np.asarray(b, dtype=np.float32)
    (xr, xi), (br, bi) = parts(x), parts(b)
    if side:
        return join((br * xr) + (bi * xi), (br * xi) - (bi * xr))
    return join((xr * br) - (xi * bi), (xr * bi) + (xi * br))


def rank_reference(h, w, s, r, o, sides="both", filt=None, offsets=None, interval=False, side=None):
    """dict(greater, equal, cands [Q] int64, bad [Q] bool, and with `interval` lo, hi [Q] int64): tests/_rank_ref.rank_reference with
    the ComplEx rule's q.  ``side`` (int array [Q]): replaces the sides of the queries -- with it (s, r, o) are taken as (anchor, rel,
    truth) directly, and a value outside {0, 1} makes the query bad."""
    h32, w32 = np.asarray(h, dtype=np.float32), np.asarray(w, dtype=np.float32)
    (N, D), R = h32.shape, w32.shape[0]
    if side is None:
        a, rr, t, head = _rank_ref.queries(s, r, o, sides)
        side = head.astype(np.int64)
    else:
        a, rr, t, side = (np.asarray(x, dtype=np.int64) for x in (s, r, o, side))
    Q = len(a)
    tails, heads = _rank_ref.known_sets(filt, N, R)
    offs = None if offsets is None else np.asarray(offsets, dtype=np.int64)
    h64 = h32.astype(np.float64)
    out = {k: np.zeros(Q, dtype=np.int64) for k in ("greater", "equal", "cands", "lo", "hi")}
    out["bad"] = np.zeros(Q, dtype=bool)
    g = (D + 1) * 2.0 ** -24 / (1 - (D + 1) * 2.0 ** -24)
    for j in range(Q):
        aj, rj, tj, sj = int(a[j]), int(rr[j]), int(t[j]), int(side[j])
        ok = 0 <= aj < N and 0 <= tj < N and 0 <= rj < R and sj in (0, 1)
        lo, hi = 0, N
        if ok and offs is not None:
            ok = offs[0] <= tj < offs[-1]
            if ok:
                ty = int(np.searchsorted(offs, tj, side="right")) - 1
                lo, hi = max(int(offs[ty]), 0), min(int(offs[ty + 1]), N)
        if not ok:
            out["bad"][j] = True
            continue
        q = rank_q(h32[aj], w32[rj], sj).astype(np.float64)  # (exact float32, then exact)
        sc = h64[lo:hi] @ q
        p = float(h64[tj] @ q)
        keep = np.ones(hi - lo, dtype=bool)
        keep[tj - lo] = False
        for c in (heads.get((rj, aj), ()) if sj else tails.get((aj, rj), ())):
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
