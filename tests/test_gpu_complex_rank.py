"""Filtered ComplEx ranking on the GPU (HET_complex_rank_prelude in front of the rank pass of csrc/triple_rank.hip, through
het_amd.linkpred.complex_rank) against the numpy reference of the rule (tests/_complex_ref.py, q in exact float32): exact on integer
grids over the tile, width, type-run and filter ladders of tests/test_gpu_rank.py on both sides; ties by bits; the fp64 interval test
on normal inputs; bad queries, a bad side included; determinism, the torch composition, poison, layouts; and the asymmetry between
the tail rank and the head rank of one triple.  Every tile size is read from kernels.triple_rank_params()."""
import functools

import numpy as np
import pytest
import torch

from tests import _complex_ref as ref
from tests import _rank_ref
from tests._poison import POISON_IDS, POISONS, poisoned

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]


@functools.lru_cache(maxsize=None)
def params():
    import het_amd.kernels as k
    return k.triple_rank_params()


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _filter(filt, N, R):
    from het_amd import linkpred as lp
    return None if filt is None else lp.FilterIndex(*(_dev(np.asarray(x, dtype=np.int64)) for x in filt), N, R)


def _rank(h, w, s, r, o, dtype=torch.float32, sides="both", filt=None, offsets=None, **kw):
    from het_amd import linkpred as lp
    return lp.complex_rank(_dev(h, dtype), _dev(w), _dev(s), _dev(r), _dev(o), sides=sides, filter=_filter(filt, h.shape[0], w.shape[0]),
                           node_type_offsets=offsets, **kw)


def _assert_same(got, want, what=""):
    for name, field in (("greater", got.greater), ("equal", got.equal), ("cands", got.candidates)):
        assert field.dtype == torch.int32 and field.is_cuda
        w = torch.from_numpy(want[name]).to(torch.int32)
        assert torch.equal(field.cpu(), w), "%s %s: got %s, want %s" % (what, name, field.cpu().tolist()[:16], w.tolist()[:16])
    assert torch.equal(got.bad.cpu(), torch.from_numpy(want["bad"])), what + " bad"


def _check(h, w, s, r, o, dtype, sides="both", filt=None, offsets=None, what=""):
    want = ref.rank_reference(h, w, s, r, o, sides, filt=filt, offsets=offsets)
    _assert_same(_rank(h, w, s, r, o, dtype, sides, filt, offsets), want, what)
    return want


# ------------------------------------------------------------------------------------------------------------ exact on integer grids
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_candidate_and_query_tile_ladders(dtype):
    C, M = params()["cand_tile"], params()["query_tile"]
    for N in (C - 1, C, C + 1, 2 * C + 1):
        h, w, s, r, o = _rank_ref.integer_case(N, 3, 8, 7, seed=N)
        _check(h, w, s, r, o, dtype, "both", what="N=%d" % N)
    for Q in (1, M - 1, M, M + 1):
        h, w, s, r, o = _rank_ref.integer_case(2 * C + 1, 3, 8, Q, seed=100 + Q)
        for sides in ("tail", "head"):
            want = _check(h, w, s, r, o, dtype, sides, what="Q=%d %s" % (Q, sides))
            assert want["equal"].sum() > 0 or Q == 1  # (the grid ties)
    h, w, s, r, o = _rank_ref.integer_case(C + 1, 3, 4, 1, seed=9)
    _check(h, w, s[:0], r[:0], o[:0], dtype, "both", what="Q=0")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("D", [4, 8, 60, 64, 68, 128, "max"])
def test_width_ladder(dtype, D):
    C, M = params()["cand_tile"], params()["query_tile"]
    D = params()["max_width"] if D == "max" else D
    h, w, s, r, o = _rank_ref.integer_case(C + 1, 4, D, M + 1, seed=D)
    filt = (s[:20], r[:20], np.arange(20) % (C + 1))
    _check(h, w, s, r, o, dtype, "both", filt=filt, what="D=%d" % D)


def test_more_queries_than_a_workgroup_keeps_and_more_tiles_than_workgroups():
    """The two sizes at which the pass takes another path: a second chunk of query tiles, and work items of more than one candidate tile."""
    p = params()
    Q = p["chunk_tiles"] * p["query_tile"] + 1
    h, w, s, r, o = _rank_ref.integer_case(p["cand_tile"] + 1, 3, 4, Q, seed=21)
    _check(h, w, s, r, o, torch.float32, "head", filt=(s[::3] // 2, r[::3], o[::3]), what="Q=%d" % Q)
    N = (p["max_blocks"] + 1) * p["cand_tile"] + 1
    h, w, s, r, o = _rank_ref.integer_case(N, 2, 4, 3, seed=22)
    o[0], o[1] = N - 1, 0
    filt = (np.repeat(s[:1], 300), np.repeat(r[:1], 300), np.arange(N - 300, N))
    _check(h, w, s, r, o, torch.bfloat16, "both", filt=filt, offsets=[0, 70, N], what="N=%d" % N)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("sides", ["both", "tail", "head"])
def test_type_runs_and_filter_lists(dtype, sides):
    """The case of tests/test_gpu_rank.py: a run boundary inside a tile, a run of one node, queries of different types in one query
    tile; filter lists that are empty, the truth only, longer than a candidate tile and a whole run; duplicates, pairs outside the
    run, a hub anchor shared by many queries."""
    C, M = params()["cand_tile"], params()["query_tile"]
    N, R, P = 2 * C + 1, 3, M + 1
    offsets = [0, C - 24, C - 23, N]
    h, w, s, r, o = _rank_ref.integer_case(N, R, 12, P, seed=31)
    hub = 5
    s[: P // 2] = hub  # a hub anchor (tail queries) ...
    o[P // 2: P // 2 + 20] = hub  # ... and a hub truth (the anchor of head queries)
    r[:10] = 0
    o[3:10] = np.arange(C, C + 7)  # tail queries (hub, r0, a node of the last run) ...
    r[P // 2: P // 2 + 6] = 0
    s[P // 2: P // 2 + 6] = np.arange(C + 10, C + 16)  # ... and head queries (a node of the last run, r0, hub)
    o[0], s[1], o[2] = C - 24, C - 24, 0  # the run of one node as truth (no candidates), as anchor
    want = _check(h, w, s, r, o, dtype, sides, offsets=offsets, what="no filter")
    one = want["cands"][0 if sides != "head" else 1]
    assert one == 0 and not want["bad"].any()
    empty = tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    _assert_same(_rank(h, w, s, r, o, dtype, sides, empty, offsets), want, "empty filter")
    _check(h, w, s, r, o, dtype, sides, filt=(s, r, o), offsets=offsets, what="truth only")
    run = np.arange(C - 23, N)  # the whole last run, longer than a candidate tile, as known tails of (hub, r0) and heads of (r0, hub)
    rng = np.random.default_rng(32)
    fs = np.concatenate([s, np.full(len(run), hub), run, np.full(30, hub), rng.integers(0, N, 200), [N, 0, 3]])
    fr = np.concatenate([r, np.zeros(len(run), dtype=np.int64), np.zeros(len(run), dtype=np.int64), np.zeros(30, dtype=np.int64),
                         rng.integers(0, R, 200), [0, R, 0]])
    fo = np.concatenate([o, run, np.full(len(run), hub), np.arange(30), rng.integers(0, N, 200), [0, 0, -1]])  # (0..29: another run)
    fs, fr, fo = (np.concatenate([x, x[:50]]) for x in (fs, fr, fo))  # duplicates
    want = _check(h, w, s, r, o, dtype, sides, filt=(fs, fr, fo), offsets=offsets, what="long lists")
    assert (want["cands"] == 0).sum() >= 5  # (the hub's queries on relation 0 with a truth in the last run have no candidate left)
    _check(h, w, s, r, o, dtype, sides, filt=(fs, fr, fo), what="long lists, one run")


def test_the_tail_rank_and_the_head_rank_of_one_triple_differ_where_the_reference_says():
    """The asymmetry: for the triples (s, r, o) with s and o swapped the DistMult ranks are those of the unswapped ones with the sides
    exchanged; the ComplEx ranks are not -- and both agree with their references count by count."""
    from het_amd import linkpred as lp
    C = params()["cand_tile"]
    N, R, D, P = 2 * C + 1, 3, 16, 50
    h, w, s, r, o = _rank_ref.integer_case(N, R, D, P, seed=71)
    want = _check(h, w, s, r, o, torch.float32, "both", what="asymmetry")
    tail, head = want["greater"][:P], want["greater"][P:]
    assert (tail != head).sum() > P // 2
    # the same triples reversed: the tail queries of (o, r, s) have the anchor and the truth of the head queries of (s, r, o)
    rev = _check(h, w, o, r, s, torch.float32, "both", what="reversed")
    assert (rev["greater"][:P] != head).any() and (rev["greater"][P:] != tail).any()
    dm = lp.distmult_rank(_dev(h), _dev(w), _dev(s), _dev(r), _dev(o))
    dm_rev = lp.distmult_rank(_dev(h), _dev(w), _dev(o), _dev(r), _dev(s))
    assert torch.equal(dm.greater[:P], dm_rev.greater[P:]) and torch.equal(dm.greater[P:], dm_rev.greater[:P])


@pytest.mark.parametrize("which", ["a", "r", "t", "side"])
def test_bad_queries_are_counted_not_asserted(which):
    import het_amd.kernels as k
    C = params()["cand_tile"]
    N, R = C + 1, 3
    h, w, s, r, o = _rank_ref.integer_case(N, R, 8, 9, seed=41)
    side = np.array([0, 1, 0, 1, 1, 0, 0, 1, 0])
    if which == "side":
        side[[2, 7]] = (2, -1)
    else:
        {"a": s, "r": r, "t": o}[which][[2, 7]] = (-1, {"a": N, "r": R, "t": N}[which])
    # the C-level wrapper takes (anchor, rel, truth, side) as they are
    want = ref.rank_reference(h, w, s, r, o, side=side)
    assert want["bad"].tolist() == [i in (2, 7) for i in range(9)]
    g, e, c, bad = k.complex_rank(_dev(h), _dev(w), _dev(s), _dev(r), _dev(o), _dev(side), None, None, None)
    assert bad.dtype == torch.int64 and int(bad) == 2  # (the count the prelude keeps on the device)
    for name, got in (("greater", g), ("equal", e), ("cands", c)):
        assert torch.equal(got.cpu(), torch.from_numpy(want[name]).to(torch.int32)), name
    assert g[[2, 7]].tolist() == [0, 0] and c[[2, 7]].tolist() == [0, 0]
    if which != "side":  # the module forms the sides itself: the other three through it, with a filter and with a node in no run
        _check(h, w, s, r, o, torch.float32, "tail", filt=(s, r, o), what="bad " + which)
        o2 = o.copy()
        o2[0] = 0
        _check(h, w, s, r, o2, torch.bfloat16, "both", offsets=[1, 9, N], what="no run")


# ------------------------------------------------------------------------------------------------------------ normal inputs
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("sides", ["tail", "head"])
def test_a_candidate_row_with_the_true_rows_bits_ties_exactly(dtype, sides):
    """The true node's row copied onto three other candidates, one of them in another tile: each copy ties with p_j exactly on both
    sides, so the MFMA scores and the prelude's fmaf chain are one arithmetic over the ComplEx q as well.  With the copies filtered
    out, greater stays and equal drops by 3."""
    C = params()["cand_tile"]
    N, R, D, Q = 2 * C + 1, 5, 64, 40
    rng = np.random.default_rng(51)
    h = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(dtype).float().numpy()
    w = rng.standard_normal((R, D)).astype(np.float32)
    t0, copies = 3, [7, C - 1, C + 9]
    h[copies] = h[t0]
    anchor, r, truth = rng.integers(C // 2, C, Q), rng.integers(0, R, Q), np.full(Q, t0)
    s, o = (anchor, truth) if sides == "tail" else (truth, anchor)
    got = _rank(h, w, s, r, o, dtype, sides)
    assert (got.equal >= 3).all(), got.equal.tolist()
    listed = (np.repeat(anchor, 3), np.repeat(r, 3), np.tile(copies, Q))
    filt = listed if sides == "tail" else (listed[2], listed[1], listed[0])
    less = _rank(h, w, s, r, o, dtype, sides, filt)
    assert torch.equal(less.greater, got.greater) and torch.equal(less.equal, got.equal - 3) and torch.equal(less.candidates, got.candidates - 3)
    want = ref.rank_reference(h, w, s, r, o, sides, interval=True)
    assert (want["lo"] <= got.greater.cpu().numpy()).all() and ((got.greater + got.equal).cpu().numpy() <= want["hi"]).all()


@pytest.mark.parametrize("case", _rank_ref.NORMAL_CASES, ids=lambda c: "D%d-N%d-Q%d-seed%d" % c)
def test_normal_inputs_against_fp64_intervals(case):
    """lo_j <= greater_j and greater_j + equal_j <= hi_j for every query of both sides, cands exact (the intervals of
    tests/_rank_ref.py around the reference's exact-float32 q)."""
    D, N, Q, seed = case
    h, w, s, r, o = _rank_ref.normal_case(D, N, Q, seed)
    want = ref.rank_reference(h, w, s, r, o, "both", interval=True)
    got = _rank(h, w, s, r, o, torch.float32, "both")
    g, e = got.greater.cpu().numpy().astype(np.int64), got.equal.cpu().numpy().astype(np.int64)
    print("queries off the fp64 count: %d of %d" % (int((g != want["greater"]).sum()), 2 * Q))
    assert (want["lo"] <= g).all() and (g + e <= want["hi"]).all()
    assert np.array_equal(got.candidates.cpu().numpy(), want["cands"]) and not got.bad.any()


# ------------------------------------------------------------------------------------------------------------ other cases
def _mixed_case():
    C, M = params()["cand_tile"], params()["query_tile"]
    N, R, P = 2 * C + 1, 4, M + 1
    h, w, s, r, o = _rank_ref.integer_case(N, R, 68, P, seed=61)
    rng = np.random.default_rng(62)
    filt = (np.concatenate([s, rng.integers(0, N, 400)]), np.concatenate([r, rng.integers(0, R, 400)]), np.concatenate([o, rng.integers(0, N, 400)]))
    return h, w, s, r, o, filt, [0, C + 3, N]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_same_bits_on_two_calls_and_equal_to_the_torch_composition(dtype):
    from het_amd import linkpred as lp
    h, w, s, r, o, filt, offs = _mixed_case()
    a = _rank(h, w, s, r, o, dtype, "both", filt, offs)
    b = _rank(h, w, s, r, o, dtype, "both", filt, offs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _rank(h, w, s, r, o, dtype, "both", filt, offs, native=False)
    d = lp.complex_rank_torch(_dev(h, dtype), _dev(w), _dev(s), _dev(r), _dev(o), filter=_filter(filt, h.shape[0], w.shape[0]),
                              node_type_offsets=offs, chunk=50)
    for x, y, z in zip(a, c, d):
        assert torch.equal(x, y) and torch.equal(x, z)
    # normal inputs: the same bits again (integer atomics only)
    hn, wn, sn, rn, on = _rank_ref.normal_case(64, 515, 70, 4)
    a, b = _rank(hn, wn, sn, rn, on, dtype), _rank(hn, wn, sn, rn, on, dtype)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
def test_poisoned_workspace_and_outputs_change_nothing(value):
    h, w, s, r, o, filt, offs = _mixed_case()
    want = ref.rank_reference(h, w, s, r, o, "both", filt=filt, offsets=offs)
    with poisoned(value) as record:
        got = _rank(h, w, s, r, o, torch.float32, "both", filt, offs)
    assert record.from_module("het_amd.kernels")  # (the workspace was taken uninitialised and filled)
    _assert_same(got, want, "poison")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_strided_and_misaligned_rows_run_on_a_copy(dtype):
    from het_amd import linkpred as lp
    h, w, s, r, o, filt, offs = _mixed_case()
    want = ref.rank_reference(h, w, s, r, o, "both", filt=filt, offsets=offs)
    F = _filter(filt, h.shape[0], w.shape[0])
    ids = (_dev(s), _dev(r), _dev(o))
    wide = torch.zeros(h.shape[0], 2 * h.shape[1], dtype=dtype, device="cuda")
    wide[:, ::2] = _dev(h, dtype)
    flat = torch.zeros(h.size + 1, dtype=dtype, device="cuda")
    flat[1:] = _dev(h, dtype).reshape(-1)
    wflat = torch.zeros(w.size + 1, device="cuda")
    wflat[1:] = _dev(w).reshape(-1)
    for ht, wt in ((wide[:, ::2], _dev(w)), (flat[1:].view(h.shape), _dev(w)), (_dev(h, dtype), wflat[1:].view(w.shape))):
        assert not ht.is_contiguous() or ht.data_ptr() % 16 or wt.data_ptr() % 16
        _assert_same(lp.complex_rank(ht, wt, *ids, filter=F, node_type_offsets=offs), want, "layout")


def test_the_decoder_ranks_under_no_grad_and_keeps_nothing():
    from het_amd import linkpred as lp
    h, w, s, r, o, filt, offs = _mixed_case()
    want = ref.rank_reference(h, w, s, r, o, "both", filt=filt, offsets=offs)
    F = _filter(filt, h.shape[0], w.shape[0])
    ids = (_dev(s), _dev(r), _dev(o))
    dec = lp.ComplExDecoder(w.shape[0], w.shape[1]).cuda()
    with torch.no_grad():
        dec.w_relation.copy_(_dev(w))
    ht = _dev(h).requires_grad_(True)
    outs = [dec.rank(ht * 1.0, *ids, filter=F, node_type_offsets=offs)]
    with torch.inference_mode():
        outs.append(dec.rank(_dev(h), *ids, filter=F, node_type_offsets=offs))
    for got in outs:
        _assert_same(got, want, "mode")
        assert all(not x.requires_grad and x.grad_fn is None for x in got)
    assert ht.grad is None
    m = lp.ranking_metrics(outs[0])
    assert m["queries"] == 2 * len(s) and 0.0 < m["mrr"] <= 1.0
