"""Filtered DistMult ranking without a GPU: the numpy reference of the rule (tests/_rank_ref.py) against a toy graph ranked by hand, the
torch composition (het_amd.linkpred.distmult_rank_torch) against the reference on integer grids, ranking_metrics on hand-made counts,
FilterIndex against a Python set construction, and the decidedness of the normal-input cases the GPU test uses."""
import math

import numpy as np
import pytest
import torch

from tests import _rank_ref as ref


def _res(out):
    return tuple(torch.from_numpy(out[k]) for k in ("greater", "equal", "cands", "bad"))


def _same(got, out):
    g, e, c, b = _res(out)
    assert torch.equal(got.greater.long().cpu(), g) and torch.equal(got.equal.long().cpu(), e)
    assert torch.equal(got.candidates.long().cpu(), c) and torch.equal(got.bad.cpu(), b)


def test_reference_on_a_toy_graph_ranked_by_hand():
    # D = 1: the score of candidate c for the query (a, r) is h[a] * w[r] * h[c]
    h = np.array([[1.], [2.], [3.], [2.], [-1.]], dtype=np.float32)
    w = np.array([[1.], [-1.]], dtype=np.float32)
    s, r, o = [0, 1], [0, 1], [1, 3]
    # tail queries: (0, r0, ?=1): scores of c = 0..4 are 1 2 3 2 -1, p = 2: without the truth greater {2}, equal {3}, 4 candidates
    #               (1, r1, ?=3): scores -2 -4 -6 -4 2, p = -4: greater {0, 4}, equal {1}
    out = ref.rank_reference(h, w, s, r, o, "tail")
    assert out["greater"].tolist() == [1, 2] and out["equal"].tolist() == [1, 1] and out["cands"].tolist() == [4, 4]
    # head queries: (?=0, r0, 1): q = 2: scores 2 4 6 4 -2, p = 2: greater {1, 2, 3}; (?=1, r1, 3): q = -2: p = -4: greater {0, 4}, equal {3}
    out = ref.rank_reference(h, w, s, r, o, "head")
    assert out["greater"].tolist() == [3, 2] and out["equal"].tolist() == [0, 1]
    both = ref.rank_reference(h, w, s, r, o, "both")
    assert both["greater"].tolist() == [1, 2, 3, 2]
    # the filter: (0, r0, 2) and (0, r0, 3) known (the second twice): the tail query 0 loses its greater and its equal candidate;
    # the head query of (0, r0, 1) is untouched by tails; (2, r0, 1) known removes head candidate 2
    filt = ([0, 0, 0, 2, 9], [0, 0, 0, 0, 0], [2, 3, 3, 1, 1])
    out = ref.rank_reference(h, w, s, r, o, "both", filt=filt)
    assert out["greater"].tolist() == [0, 2, 2, 2] and out["equal"].tolist() == [0, 1, 0, 1] and out["cands"].tolist() == [2, 4, 3, 4]
    # types {0, 1, 2} and {3, 4}: query 0 ranks in the first run, query 1 in the second; a run of one node has no candidates
    out = ref.rank_reference(h, w, s, r, o, "tail", offsets=[0, 3, 5])
    assert out["greater"].tolist() == [1, 1] and out["equal"].tolist() == [0, 0] and out["cands"].tolist() == [2, 1]
    out = ref.rank_reference(h, w, [0], [0], [4], "tail", offsets=[0, 4, 5])
    assert out["cands"].tolist() == [0] and not out["bad"][0]
    # bad: each id alone, and a true node in no run
    out = ref.rank_reference(h, w, [5, 0, 0, 0, -1], [0, 2, 0, 0, 0], [1, 1, 5, 0, 1], "tail", offsets=[1, 3, 5])
    assert out["bad"].tolist() == [True, True, True, True, True] and out["cands"].sum() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.float16])
@pytest.mark.parametrize("sides", ["both", "tail", "head"])
def test_torch_fallback_equals_the_reference_on_integer_grids(dtype, sides):
    from het_amd import linkpred as lp
    N, R, D, P = 97, 4, 12, 41
    h, w, s, r, o = ref.integer_case(N, R, D, P, seed=5)
    s[3], r[4], o[5] = N, -1, -7  # bad ids
    rng = np.random.default_rng(6)
    filt = (np.concatenate([s, rng.integers(0, N, 300), [N, 0]]), np.concatenate([r, rng.integers(0, R, 300), [0, R]]),
            np.concatenate([o, rng.integers(0, N, 300), [0, 0]]))
    offs = [0, 30, 31, 97]
    ht, wt = torch.from_numpy(h).to(dtype), torch.from_numpy(w).to(dtype if dtype == torch.float64 else torch.float32)
    ids = tuple(torch.from_numpy(x) for x in (s, r, o))
    F = lp.FilterIndex(*(torch.from_numpy(x) for x in filt), N, R)
    for kw, rk in ((dict(), dict()), (dict(filter=F), dict(filt=filt)), (dict(filter=F, node_type_offsets=offs), dict(filt=filt, offsets=offs))):
        want = ref.rank_reference(h, w, s, r, o, sides, **rk)
        _same(lp.distmult_rank_torch(ht, wt, *ids, sides=sides, chunk=40, **kw), want)
        _same(lp.distmult_rank(ht, wt, *ids, sides=sides, **kw), want)  # (CPU tensors take the composition)
        _same(lp.distmult_rank(ht, wt, *ids, sides=sides, native=False, **kw), want)
    dec = lp.DistMultDecoder(R, D)
    with torch.no_grad():
        dec.w_relation.copy_(torch.from_numpy(w))
    got = dec.rank(ht.float().requires_grad_(True), *ids, sides=sides, filter=F)
    _same(got, ref.rank_reference(h, w, s, r, o, sides, filt=filt))
    assert got.greater.dtype == torch.int32 and not got.greater.requires_grad and got.greater.grad_fn is None
    with pytest.raises(ValueError):
        lp.distmult_rank(ht, wt, *ids, sides="all")
    with pytest.raises(ValueError):
        lp.distmult_rank(ht, wt, *ids, filter=lp.FilterIndex(*ids, N + 1, R))
    with pytest.raises(ValueError):
        dec.rank(ht[:, :8].float(), *ids)


def test_ranking_metrics_on_hand_made_counts():
    from het_amd import linkpred as lp
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    # ranks 1, 2.5 (three ties: 1 + 0 + 3 / 2), 4, 11; one bad query (left out)
    res = lp.RankResult(i32([0, 0, 3, 10, 0]), i32([0, 3, 0, 0, 0]), i32([9, 9, 9, 20, 0]), torch.tensor([False, False, False, False, True]))
    m = lp.ranking_metrics(res)
    assert m["queries"] == 4 and set(m) == {"mrr", "mean_rank", "hits@1", "hits@3", "hits@10", "queries"}
    assert m["mrr"] == pytest.approx((1 + 1 / 2.5 + 1 / 4 + 1 / 11) / 4, rel=1e-15) and m["mean_rank"] == pytest.approx(18.5 / 4, rel=1e-15)
    assert m["hits@1"] == 0.25 and m["hits@3"] == 0.5 and m["hits@10"] == 0.75
    assert lp.ranking_metrics(res, ks=(4, 11)) == {"mrr": m["mrr"], "mean_rank": m["mean_rank"], "hits@4": 0.75, "hits@11": 1.0, "queries": 4}
    # a run of one node: no candidate, rank 1, not bad
    m = lp.ranking_metrics(lp.RankResult(i32([0]), i32([0]), i32([0]), torch.tensor([False])))
    assert m["mrr"] == 1.0 and m["queries"] == 1
    m = lp.ranking_metrics(lp.RankResult(i32([0]), i32([0]), i32([0]), torch.tensor([True])))
    assert m["queries"] == 0 and math.isnan(m["mrr"]) and math.isnan(m["hits@10"])
    assert lp.RankResult._fields == ("greater", "equal", "candidates", "bad")


def test_filter_index_pairs_equal_a_set_construction():
    from het_amd import linkpred as lp
    rng = np.random.default_rng(11)
    N, R, E = 23, 3, 400
    fs, fr, fo = rng.integers(-1, N + 1, E), rng.integers(-1, R + 1, E), rng.integers(-1, N + 1, E)  # duplicates and ids out of range
    F = lp.FilterIndex(torch.from_numpy(fs), torch.from_numpy(fr), torch.from_numpy(fo), N, R)
    ok = (fs >= 0) & (fs < N) & (fo >= 0) & (fo < N) & (fr >= 0) & (fr < R)
    assert F.tail_keys.shape[0] == F.head_keys.shape[0] == int(ok.sum())  # duplicates are kept
    assert torch.equal(F.tail_keys, torch.sort(F.tail_keys).values) and torch.equal(F.head_keys, torch.sort(F.head_keys).values)
    assert set(zip(F.tail_keys.tolist(), F.tail_vals.tolist())) == {(r * N + s, o) for s, r, o in zip(fs[ok].tolist(), fr[ok].tolist(), fo[ok].tolist())}
    assert set(zip(F.head_keys.tolist(), F.head_vals.tolist())) == {(r * N + o, s) for s, r, o in zip(fs[ok].tolist(), fr[ok].tolist(), fo[ok].tolist())}
    a, r = rng.integers(-1, N + 1, 60), rng.integers(-1, R + 1, 60)
    head = rng.integers(0, 2, 60).astype(bool)
    pq, pc = F.pairs(torch.from_numpy(a), torch.from_numpy(r), torch.from_numpy(head))
    assert pq.dtype == pc.dtype == torch.int64 and pq.shape == pc.shape and torch.equal(pq, torch.sort(pq).values)
    want = ref.filter_pairs((fs, fr, fo), a, r, head, N, R)
    assert set(zip(pq.tolist(), pc.tolist())) == want and len(pq) >= len(want)
    e = lp.FilterIndex(*(torch.zeros(0, dtype=torch.int64),) * 3, N, R)
    pq, pc = e.pairs(torch.from_numpy(a), torch.from_numpy(r), torch.from_numpy(head))
    assert pq.numel() == pc.numel() == 0
    with pytest.raises(ValueError):
        lp.FilterIndex(torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), N, R)


@pytest.mark.parametrize("case", ref.NORMAL_CASES, ids=lambda c: "D%d-N%d-Q%d-seed%d" % c)
def test_normal_cases_are_decided_on_the_reference_alone(case):
    """At least 85 % of the queries have lo == hi and no interval is wider than 2: the fp64 bounds pin the counts the GPU test
    compares, whatever the kernels give.  A seed that misses is replaced, not excused."""
    D, N, Q, seed = case
    h, w, s, r, o = ref.normal_case(D, N, Q, seed)
    out = ref.rank_reference(h, w, s, r, o, "tail", interval=True)
    width = out["hi"] - out["lo"]
    print("decided share %.1f %%, widest interval %d" % (100.0 * (width == 0).mean(), width.max()))
    assert (width >= 0).all() and (width == 0).mean() >= 0.85 and width.max() <= 2
    assert (out["lo"] <= out["greater"]).all() and (out["greater"] + out["equal"] <= out["hi"]).all()
