"""The link-prediction rule without a GPU: the torch CPU path of het_amd/linkpred.py against the independent numpy restatement
(tests/_triple_ref.py) -- keyed corruptions bit for bit, their uniformity, the keyed positive edges, and the torch composition of the
DistMult head against the fp64 reference.  Fails on a tree without the feature (het_amd.linkpred does not exist)."""
import numpy as np
import pytest
import torch

from tests import _triple_ref as ref
from tests.util import ROW_LADDER, assert_close, random_graph

SEEDS = (1, 2 ** 40 + 17, 2 ** 64 - 3)
BIG = 2 ** 31 - 1


def _positives(P, N, R, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, N, P), rng.integers(0, R, P), rng.integers(0, N, P)


def _torch_corruptions(src, rel, dst, K, seed, draw, N, offsets=None):
    from het_amd.linkpred import keyed_corruptions
    out = keyed_corruptions(torch.tensor(src), torch.tensor(rel), torch.tensor(dst), K, seed=seed, draw=draw,
                            node_type_offsets=None if offsets is None else torch.tensor(offsets), num_nodes=N)
    assert all(t.dtype == torch.int64 and t.shape == (len(src) * (1 + K),) for t in out)
    return [t.numpy() for t in out]


# (num_nodes, node_type_offsets): no offsets; runs of 40, 1 (always that node), 0 and 59 nodes; one span of 2^31 - 1
LAYOUTS = ((100, None), (100, (0, 40, 41, 41, 100)), (BIG, None), (BIG, (0, BIG)))


@pytest.mark.parametrize("K", (0, 1, 5))
@pytest.mark.parametrize("seed", SEEDS)
def test_corruptions_equal_the_numpy_rule_bit_for_bit(seed, K):
    for N, offsets in LAYOUTS:
        for P in ROW_LADDER:
            src, rel, dst = _positives(P, N, 7, P + K)
            if offsets is not None and N == 100 and P:
                src[0], dst[0] = 40, 40  # the run of one node
            got = _torch_corruptions(src, rel, dst, K, seed, 3, N, offsets)
            s, r, o, side = ref.corruptions(src, rel, dst, K, seed, 3, N, offsets)
            for name, a, b in zip("sro", got, (s, r, o)):
                assert np.array_equal(a, b), f"{name} at P={P} K={K} N={N} offsets={offsets}"
            assert np.array_equal(s[:P], src) and np.array_equal(o[:P], dst) and np.array_equal(r, np.concatenate([rel, np.repeat(rel, K)]))
            # exactly one end of a corruption is drawn; it stays inside the run (the type) of the end it replaces
            i = np.arange(P * K) // max(K, 1)
            assert np.array_equal(np.where(side == 1, o[P:], s[P:]), np.where(side == 1, dst[i], src[i]))
            new, old = np.where(side == 1, s[P:], o[P:]), np.where(side == 1, src[i], dst[i])
            assert ((new >= 0) & (new < N)).all()
            if offsets is not None:
                edges = np.asarray(offsets)
                assert np.array_equal(np.searchsorted(edges, new, side="right"), np.searchsorted(edges, old, side="right"))
            if offsets is not None and N == 100 and P and K:
                assert (np.where(side[:K] == 1, s[P:P + K], o[P:P + K]) == 40).all()  # a run of length 1: always that node


def test_seed_and_draw_each_change_the_sample_and_sides_are_about_half():
    P, K, N = 2048, 5, 10 ** 6
    src, rel, dst = _positives(P, N, 3, 0)
    base = _torch_corruptions(src, rel, dst, K, 11, 0, N)
    again = _torch_corruptions(src, rel, dst, K, 11, 0, N)
    other_draw = _torch_corruptions(src, rel, dst, K, 11, 1, N)
    other_seed = _torch_corruptions(src, rel, dst, K, 12, 0, N)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for other in (other_draw, other_seed):
        assert (np.concatenate(base) != np.concatenate(other)).mean() > 0.3  # (a third of all ids are the replaced ends)
    head = base[0][P:] != np.repeat(src, K)  # the head was replaced (a draw of the old node itself has probability 1e-6)
    assert abs(head.mean() - 0.5) < 5 * 0.5 / np.sqrt(P * K)
    # out-of-table ends are copied as they are, whatever side is drawn
    bad = _torch_corruptions(np.array([-1, N]), np.array([0, 0]), np.array([N + 5, -7]), 4, 1, 0, N)
    assert set(bad[0][2:]) <= {-1, N} and set(bad[2][2:]) <= {N + 5, -7}


def test_uniformity_of_the_replacement():
    """Deterministic: P K = 200 000 draws into a run of ``span`` nodes for three seeds and spans 2, 7 and 1000; every node's count lies
    within 5 binomial standard deviations of its expectation.  Worst observed: 3.61 standard deviations (span 1000, seed 3); the rule's
    own bias is below span / 2^32 per node, 2.3e-7 of a count's expectation at most here."""
    from het_amd.linkpred import keyed_corruptions
    P, K, lo = 1000, 200, 5
    for span in (2, 7, 1000):
        offsets = (0, lo, lo + span, lo + span + 3)
        for seed in (1, 2, 3):
            ends = np.full(P, lo)
            s, _, o, side = ref.corruptions(ends, np.zeros(P, dtype=np.int64), ends, K, seed, 0, offsets[-1], offsets)
            t = keyed_corruptions(torch.tensor(ends), torch.zeros(P, dtype=torch.int64), torch.tensor(ends), K, seed=seed, draw=0,
                                  node_type_offsets=torch.tensor(offsets), num_nodes=offsets[-1])
            assert np.array_equal(t[0].numpy(), s) and np.array_equal(t[2].numpy(), o)
            new = np.where(side == 1, s[P:], o[P:]) - lo
            assert new.min() >= 0 and new.max() < span
            n, p = P * K, 1.0 / span
            dev = np.abs(np.bincount(new, minlength=span) - n * p).max() / np.sqrt(n * p * (1 - p))
            print(f"span {span} seed {seed}: worst count {dev:.2f} standard deviations from its expectation")
            assert dev <= 5.0, (span, seed, dev)


def test_keyed_positive_edges_against_numpy():
    from het_amd.linkpred import keyed_positive_edges
    g = random_graph(seed=3, n=257, r=5, e=3001)
    coo = g.get_separate_coo_original()
    E = g.get_num_edges()
    rel_of = np.repeat(np.arange(g.get_num_rels()), np.diff(coo["rel_ptrs"].numpy()))
    for seed, draw, P in ((0, 0, 1), (5, 2, 1024), (2 ** 63 + 1, 7, 4097), (9, 1, 0)):
        src, rel, dst = keyed_positive_edges(g, P, seed=seed, draw=draw)
        e = ref.positive_positions(seed, draw, P, E)
        assert ((e >= 0) & (e < E)).all()
        assert np.array_equal(src.numpy(), coo["row_indices"].numpy()[e]) and np.array_equal(dst.numpy(), coo["col_indices"].numpy()[e])
        assert np.array_equal(rel.numpy(), rel_of[e])
    a = keyed_positive_edges(g, 512, seed=1, draw=0)[0]
    assert not torch.equal(a, keyed_positive_edges(g, 512, seed=1, draw=1)[0]) and not torch.equal(a, keyed_positive_edges(g, 512, seed=2, draw=0)[0])
    hist = np.bincount(ref.positive_positions(4, 0, 30010, E), minlength=E)  # with replacement, about uniform: 10 draws per edge
    assert hist.max() <= 10 + 6 * np.sqrt(10) and (hist > 0).mean() > 0.99


def _case(N, R, T, D, seed, bad=True):
    rng = np.random.default_rng(seed)
    h, w, g = rng.standard_normal((N, D)), rng.standard_normal((R, D)), rng.standard_normal(T)
    s, r, o = rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)
    o[::7] = s[::7]  # self-pairs: both terms of grad_h land on one row
    if bad:
        s[3], o[5], r[8], r[11] = -1, N, R, -5
    return h, w, g, s, r, o


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64, torch.bfloat16), ids=("fp32", "fp64", "bf16"))
def test_torch_composition_against_the_fp64_reference(dtype):
    from het_amd.linkpred import DistMultDecoder, link_prediction_loss
    N, R, T, D = 41, 5, 301, 10
    h, w, g, s, r, o = _case(N, R, T, D, 1)
    ht = torch.tensor(h).to(dtype)
    dec = DistMultDecoder(R, D)
    with torch.no_grad():
        dec.w_relation.copy_(torch.tensor(w))
    w32 = dec.w_relation.detach().double().numpy()
    h64 = ht.double().numpy()
    x = ht.clone().requires_grad_(True)
    assert not dec.takes_native(x)
    score = dec(x, torch.tensor(s), torch.tensor(r), torch.tensor(o))
    assert score.dtype == torch.float32 and score.shape == (T,) and int(dec.last_bad) == 4
    score.backward(torch.tensor(g, dtype=torch.float32))
    g32 = torch.tensor(g, dtype=torch.float32).double().numpy()
    want = ref.scores(h64, w32, s, r, o)
    want_gh, want_gw = ref.grads(h64, w32, s, r, o, g32)
    assert_close(score, torch.tensor(want), what="score")
    assert score[[3, 5, 8, 11]].tolist() == [0.0] * 4
    assert x.grad.dtype == dtype and x.grad.shape == (N, D)
    if dtype == torch.bfloat16:
        bound = 2.0 ** -8 * np.abs(want_gh) + 1e-5 * np.abs(want_gh).max()
        assert (np.abs(x.grad.double().numpy() - want_gh) <= bound).all()  # (the project's bf16 rule: rounded once)
    else:
        assert_close(x.grad, torch.tensor(want_gh), what="grad_h")
    assert_close(dec.w_relation.grad, torch.tensor(want_gw), what="grad_w")
    with pytest.raises(ValueError, match="4 triple"):
        DistMultDecoder(R, D, check_ids=True)(ht, torch.tensor(s), torch.tensor(r), torch.tensor(o))
    # the loss: BCE with logits against labels that are the position
    sc = torch.tensor(want[:12], dtype=torch.float32)
    lab = torch.tensor([1.0] * 4 + [0.0] * 8)
    assert torch.equal(link_prediction_loss(sc, 4), torch.nn.functional.binary_cross_entropy_with_logits(sc, lab))
    with pytest.raises(ValueError):
        link_prediction_loss(sc, 13)


def test_staged_emulation_is_the_reference_up_to_fp32_rounding():
    """The fp32 emulation of the kernels' order (chunks of L and of the grad_w chunk, a hub beyond 4 L) against the fp64 sums."""
    N, R, T, D, L, C = 37, 3, 900, 8, 16, 32
    h, w, g, s, r, o = _case(N, R, T, D, 2)
    o[:4 * L + 3] = 0  # a hub
    gh, gw = ref.grads(h.astype(np.float32), w.astype(np.float32), s, r, o, g.astype(np.float32))
    sh, sw = ref.staged_grads(h, w, s, r, o, g, L, C)
    assert sh.dtype == np.float32 and sw.dtype == np.float32
    nodes, rels = ref.slot_lists(s, r, o, N, R)
    n_good = int(ref.good(s, r, o, N, R).sum())
    assert n_good < T and len(nodes[0]) > 4 * L and sum(len(x) for x in nodes) == 2 * n_good and sum(len(x) for x in rels) == n_good
    assert all(x == sorted(x) for x in nodes + rels)
    np.testing.assert_allclose(sh, gh, rtol=0, atol=2e-5 * np.abs(gh).max())
    np.testing.assert_allclose(sw, gw, rtol=0, atol=2e-5 * np.abs(gw).max())
    # on integer grids every order gives the same bits
    rng = np.random.default_rng(0)
    hi, wi, gi = rng.integers(-2, 3, (N, D)), rng.integers(-1, 3, (R, D)), rng.choice([1, -1, 2, -2, 0.5, -0.5], T)
    eh, ew = ref.staged_grads(hi, wi, s, r, o, gi, L, C)
    xh, xw = ref.grads(hi, wi, s, r, o, gi)
    assert np.array_equal(eh, xh.astype(np.float32)) and np.array_equal(ew, xw.astype(np.float32))
