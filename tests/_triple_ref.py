"""The link-prediction rule of het_amd/linkpred.py restated independently in numpy: uint64 for the keys, fp64 for the floats, and an
fp32 staged emulation of the two gradient sums in the order the kernels state (csrc/triple_score.hip).  No torch, no het_amd import."""
import numpy as np

U64 = np.uint64


def sm(z):
    """The 64-bit mixer of the keyed streams on a uint64 array or scalar (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U64) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def stream(seed, draw):
    return sm(U64(seed & (2 ** 64 - 1)) ^ sm(U64(draw & (2 ** 64 - 1))))


def keys(seed, draw, count):
    with np.errstate(over="ignore"):
        return sm(stream(seed, draw) + np.arange(count, dtype=U64))


def corruptions(src, rel, dst, K, seed, draw, num_nodes, offsets=None):
    """(s, r, o, side) of the rule: int64 arrays [P (1 + K)] and the side bit of every corruption [P K]."""
    src, rel, dst = (np.asarray(a, dtype=np.int64) for a in (src, rel, dst))
    P = src.shape[0]
    key = keys(seed, draw, P * K)
    side = (key >> U64(63)).astype(np.int64)
    u = (key >> U64(31)) & U64(0xFFFFFFFF)
    i = np.arange(P * K) // max(K, 1)
    v_old = np.where(side == 1, src[i], dst[i])
    if offsets is None:
        lo, hi = np.zeros_like(v_old), np.full_like(v_old, num_nodes)
        inside = (v_old >= 0) & (v_old < num_nodes)
    else:
        offsets = np.asarray(offsets, dtype=np.int64)
        inside = (v_old >= offsets[0]) & (v_old < offsets[-1])
        ty = np.clip(np.searchsorted(offsets[:-1], v_old, side="right") - 1, 0, len(offsets) - 2)
        lo, hi = offsets[ty], offsets[ty + 1]
    v_new = np.where(inside, lo + ((u * (hi - lo).astype(U64)) >> U64(32)).astype(np.int64), v_old)
    s = np.concatenate([src, np.where(side == 1, v_new, src[i])])
    o = np.concatenate([dst, np.where(side == 1, dst[i], v_new)])
    return s, np.concatenate([rel, rel[i]]), o, side


def positive_positions(seed, draw, count, num_edges):
    u = (keys(seed, draw, count) >> U64(31)) & U64(0xFFFFFFFF)
    return ((u * U64(num_edges)) >> U64(32)).astype(np.int64)


def good(s, r, o, N, R):
    return (s >= 0) & (s < N) & (o >= 0) & (o < N) & (r >= 0) & (r < R)


def scores(h, w, s, r, o):
    """fp64 scores [T]; +0 for a triple with an id outside its table."""
    h, w = np.asarray(h, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ok = good(s, r, o, h.shape[0], w.shape[0])
    out = np.zeros(len(s))
    out[ok] = (h[s[ok]] * w[r[ok]] * h[o[ok]]).sum(-1)
    return out


def grads(h, w, s, r, o, g):
    """(grad_h [N, D], grad_w [R, D]) in fp64."""
    h, w, g = np.asarray(h, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    ok = good(s, r, o, h.shape[0], w.shape[0])
    s, r, o, g = s[ok], r[ok], o[ok], g[ok]
    gh, gw = np.zeros_like(h), np.zeros_like(w)
    np.add.at(gh, s, g[:, None] * w[r] * h[o])
    np.add.at(gh, o, g[:, None] * w[r] * h[s])
    np.add.at(gw, r, g[:, None] * h[s] * h[o])
    return gh, gw


def slot_lists(s, r, o, N, R):
    """Per node the ascending slots 2 j + side it owns (side 0: the head s_j, side 1: the tail o_j), per relation its triples in
    ascending j; bad triples are in no list."""
    ok = good(s, r, o, N, R)
    nodes = [[] for _ in range(N)]
    rels = [[] for _ in range(R)]
    for j in np.nonzero(ok)[0]:
        nodes[s[j]].append(2 * j)
        nodes[o[j]].append(2 * j + 1)
        rels[r[j]].append(j)
    return nodes, rels


def staged_grads(h, w, s, r, o, g, L, rel_chunk):
    """The two sums in fp32 in the kernels' stated order: per node the terms (g_j * w[r_j]) * h[other end] added one by one in ascending
    slot from +0, a list longer than L in chunks of L from its start with the chunk sums added in chunk order; per relation the terms
    (h[s_j] * h[o_j]) * g_j in ascending j in chunks of ``rel_chunk``, the chunk sums in chunk order.  Every product and every add is
    rounded to fp32 (no fused multiply-add)."""
    f = np.float32
    h, w, g = np.asarray(h, dtype=f), np.asarray(w, dtype=f), np.asarray(g, dtype=f)
    N, R = h.shape[0], w.shape[0]
    nodes, rels = slot_lists(s, r, o, N, R)
    gh, gw = np.zeros_like(h), np.zeros_like(w)

    def run(terms):
        acc = np.zeros(h.shape[1], dtype=f)
        for t in terms:
            acc = acc + t
        return acc

    def chunked(items, term, size, always):
        if len(items) <= size and not always:
            return run(term(e) for e in items)
        return run(run(term(e) for e in items[c:c + size]) for c in range(0, len(items), size))

    for v, slots in enumerate(nodes):
        gh[v] = chunked(slots, lambda e: (g[e >> 1] * w[r[e >> 1]]) * h[s[e >> 1] if e & 1 else o[e >> 1]], L, False)
    for rel, js in enumerate(rels):
        gw[rel] = chunked(js, lambda j: (h[s[j]] * h[o[j]]) * g[j], rel_chunk, True)
    return gh, gw

