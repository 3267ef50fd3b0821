"""The ComplEx rule without a GPU: the numpy restatement (tests/_complex_ref.py) against itself and against the torch composition of
het_amd/linkpred.py (the CPU and odd-dtype route) -- exact on integer grids in fp32 and bf16, gradcheck in fp64, the identities that
tie ComplEx to DistMult and that make it asymmetric, the two-sided q of the ranking rule, the staged fp32 emulation, and the torch
ranking composition against the rank reference.  Fails on a tree without the feature (the symbols do not exist)."""
import numpy as np
import pytest
import torch

from tests import _complex_ref as ref
from tests import _rank_ref, _triple_ref

DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("fp32", "bf16")


def _grid_case(N, R, T, D, seed):
    """h in -2..2, w in {-1, 0, 1, 2}, g in {+-1, +-2, +-0.5}: exact in fp32 and bf16, every partial sum far below 2^24."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-2, 3, size=(N, D)).astype(np.float64)
    w = rng.integers(-1, 3, size=(R, D)).astype(np.float64)
    g = rng.choice(np.array([1, -1, 2, -2, 0.5, -0.5]), size=T)
    s, r, o = rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)
    o[::7] = s[::7]  # (self-pairs: both slots)
    assert 2 * T * 4 * 2 * 2 * 2 * D < 2 ** 24
    return h, w, g, s, r, o


def test_reference_states_the_score_two_ways_and_its_gradients_are_the_derivatives():
    h, w, g, s, r, o = _grid_case(11, 3, 40, 8, 0)
    assert np.array_equal(ref.scores(h, w, s, r, o), ref.scores_by_complex_numbers(h, w, s, r, o))
    rng = np.random.default_rng(1)
    h, w = rng.standard_normal((11, 8)), rng.standard_normal((3, 8))
    gh, gw = ref.grads(h, w, s, r, o, g)
    eps = 1e-6
    for table, grad, at in ((h, gh, (4, 3)), (h, gh, (0, 6)), (w, gw, (1, 2)), (w, gw, (2, 5))):
        keep = table[at]
        table[at] = keep + eps
        up = (ref.scores(h, w, s, r, o) * g).sum()
        table[at] = keep - eps
        down = (ref.scores(h, w, s, r, o) * g).sum()
        table[at] = keep
        assert abs((up - down) / (2 * eps) - grad[at]) < 1e-6 * max(1.0, abs(grad[at]))
    # ids outside the tables: score +0, no gradient
    s2, r2, o2 = s.copy(), r.copy(), o.copy()
    s2[0], r2[1], o2[2] = -1, 3, 11
    sc = ref.scores(h, w, s2, r2, o2)
    assert sc[:3].tolist() == [0.0, 0.0, 0.0] and np.array_equal(sc[3:], ref.scores(h, w, s, r, o)[3:])
    g0 = g.copy()
    g0[:3] = 0
    for a, b in zip(ref.grads(h, w, s2, r2, o2, g), ref.grads(h, w, s, r, o, g0)):
        assert np.allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_torch_composition_equals_the_reference_on_integer_grids(dtype):
    from het_amd.linkpred import ComplExDecoder, complex_score_torch
    for N, R, T, D, seed in ((13, 3, 60, 4, 2), (50, 5, 300, 36, 3), (7, 1, 0, 8, 4)):
        h, w, g, s, r, o = _grid_case(N, R, T, D, seed)
        if T:
            s[1], r[2] = N, -1  # (two bad triples)
        x = torch.tensor(h).to(dtype).requires_grad_(True)
        wt = torch.tensor(w, dtype=torch.float32, requires_grad=True)
        ids = [torch.tensor(a) for a in (s, r, o)]
        score, bad = complex_score_torch(x, wt, *ids)
        assert score.dtype == torch.float32 and bad.tolist() == [2 if T else 0]
        assert torch.equal(score.detach(), torch.tensor(ref.scores(h, w, s, r, o)).float())
        score.backward(torch.tensor(g, dtype=torch.float32))
        gh, gw = ref.grads(h, w, s, r, o, g)
        assert x.grad.dtype == dtype and torch.equal(x.grad, torch.tensor(gh).to(dtype)) and torch.equal(wt.grad, torch.tensor(gw).float())
        # the module on CPU tensors takes the same composition
        dec = ComplExDecoder(R, D)
        with torch.no_grad():
            dec.w_relation.copy_(wt)
        assert not dec.takes_native(x) and torch.equal(dec(x.detach(), *ids), score.detach()) and dec.last_bad.tolist() == bad.tolist()


def test_gradcheck_of_the_torch_composition_in_fp64():
    from het_amd.linkpred import complex_score_torch
    N, R, T, D = 7, 2, 9, 4
    rng = np.random.default_rng(5)
    h = torch.tensor(rng.standard_normal((N, D)), requires_grad=True)
    w = torch.tensor(rng.standard_normal((R, D)), requires_grad=True)
    s, r, o = (torch.tensor(rng.integers(0, n, T)) for n in (N, R, N))
    o[3] = s[3]
    assert torch.autograd.gradcheck(lambda a, b: complex_score_torch(a, b, s, r, o)[0], (h, w))
    assert complex_score_torch(h, w, s, r, o)[0].dtype == torch.float64


def test_identities_with_distmult_and_the_asymmetry():
    from het_amd.linkpred import complex_score_torch, distmult_score_torch
    h, w, _, s, r, o = _grid_case(17, 4, 200, 12, 6)
    ht = torch.tensor(h, dtype=torch.float32)
    ids = [torch.tensor(a) for a in (s, r, o)]
    rev = [ids[2], ids[1], ids[0]]
    # Im(w) = 0: DistMult with each real weight written into both columns of its component
    w_re = w.copy()
    w_re[:, 1::2] = 0
    both = np.repeat(w[:, 0::2], 2, axis=1)
    a = complex_score_torch(ht, torch.tensor(w_re, dtype=torch.float32), *ids)[0]
    b = distmult_score_torch(ht, torch.tensor(both, dtype=torch.float32), *ids)[0]
    assert torch.equal(a, b) and bool(a.any())
    assert np.array_equal(ref.scores(h, w_re, s, r, o), _triple_ref.scores(h, both, s, r, o))
    # Re(w) = 0: antisymmetric
    w_im = w.copy()
    w_im[:, 0::2] = 0
    wt = torch.tensor(w_im, dtype=torch.float32)
    fwd, bwd = complex_score_torch(ht, wt, *ids)[0], complex_score_torch(ht, wt, *rev)[0]
    assert torch.equal(fwd, -bwd) and bool(fwd.any())
    assert np.array_equal(ref.scores(h, w_im, s, r, o), -ref.scores(h, w_im, o, r, s))
    # in general: a triple and its reverse score differently -- the property the head exists for (a fixed case)
    hh = np.array([[1.0, 2.0, 0.0, 1.0], [2.0, -1.0, 1.0, 1.0]])
    ww = np.array([[1.0, 1.0, 2.0, -1.0]])
    z, one = np.array([0]), np.array([1])
    assert ref.scores(hh, ww, z, z, one)[0] == -2.0 and ref.scores(hh, ww, one, z, z)[0] == 6.0  # (worked by hand)
    tri = (torch.tensor(hh, dtype=torch.float32), torch.tensor(ww, dtype=torch.float32))
    assert complex_score_torch(*tri, torch.tensor(z), torch.tensor(z), torch.tensor(one))[0].tolist() == [-2.0]
    assert complex_score_torch(*tri, torch.tensor(one), torch.tensor(z), torch.tensor(z))[0].tolist() == [6.0]
    assert distmult_score_torch(*tri, torch.tensor(z), torch.tensor(z), torch.tensor(one))[0].tolist() == \
        distmult_score_torch(*tri, torch.tensor(one), torch.tensor(z), torch.tensor(z))[0].tolist()


def test_rank_q_of_both_sides_reproduces_the_scores_on_integer_grids():
    h, w, _, s, r, o = _grid_case(19, 3, 50, 8, 7)
    N = h.shape[0]
    cand = np.arange(N)
    for j in range(len(s)):
        tail_q = ref.rank_q(h[s[j]], w[r[j]], 0).astype(np.float64)
        head_q = ref.rank_q(h[o[j]], w[r[j]], 1).astype(np.float64)
        assert np.array_equal(h @ tail_q, ref.scores(h, w, np.full(N, s[j]), np.full(N, r[j]), cand))  # score(a, r, c)
        assert np.array_equal(h @ head_q, ref.scores(h, w, cand, np.full(N, r[j]), np.full(N, o[j])))  # score(c, r, a)
    # three roundings per element, none fused: a case where the fused form differs
    x = np.array([1 + 2.0 ** -12, 1 + 2.0 ** -12], dtype=np.float32)
    b = np.array([1 + 2.0 ** -12, 1.0], dtype=np.float32)
    q = ref.rank_q(x, b, 0)
    fused = np.float32(np.float64(x[0]) * np.float64(b[0]) - np.float64(np.float32(x[1] * b[1])))
    assert q.dtype == np.float32 and q[0] == np.float32(np.float32(x[0] * b[0]) - np.float32(x[1] * b[1])) and q[0] != fused


def test_staged_emulation_follows_the_fp64_gradients():
    rng = np.random.default_rng(8)
    N, R, T, D, L = 9, 2, 120, 8, 16
    h, w, g = rng.standard_normal((N, D)), rng.standard_normal((R, D)), rng.standard_normal(T)
    s, r, o = rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)
    s[5] = -1
    gh, gw = ref.grads(h, w, s, r, o, g)
    eh, ew = ref.staged_grads(h, w, s, r, o, g, L, 32)
    assert eh.dtype == np.float32 and np.abs(eh - gh).max() < 1e-4 and np.abs(ew - gw).max() < 1e-4 and np.abs(eh - gh).max() > 0
    # on an integer grid the emulation is the exact sum, whatever the chunking
    h, w, g, s, r, o = _grid_case(9, 2, 200, 8, 9)
    gh, gw = ref.grads(h, w, s, r, o, g)
    for L, rc in ((4, 8), (1000, 1000)):
        eh, ew = ref.staged_grads(h, w, s, r, o, g, L, rc)
        assert np.array_equal(eh, gh) and np.array_equal(ew, gw)


@pytest.mark.parametrize("sides", ("both", "tail", "head"))
def test_torch_ranking_composition_equals_the_rank_reference(sides):
    from het_amd import linkpred as lp
    N, R, D, P = 131, 3, 12, 40
    h, w, s, r, o = _rank_ref.integer_case(N, R, D, P, seed=10)
    s[3], r[4], o[5] = -1, R, N
    rng = np.random.default_rng(11)
    filt = (np.concatenate([s, rng.integers(0, N, 300)]), np.concatenate([r, rng.integers(0, R, 300)]), np.concatenate([o, rng.integers(0, N, 300)]))
    offs = [0, 40, 41, N]
    want = ref.rank_reference(h, w, s, r, o, sides, filt=filt, offsets=offs)
    F = lp.FilterIndex(*(torch.tensor(x) for x in filt), N, R)
    args = (torch.tensor(h), torch.tensor(w), torch.tensor(s), torch.tensor(r), torch.tensor(o))
    dec = lp.ComplExDecoder(R, D)
    with torch.no_grad():
        dec.w_relation.copy_(args[1])
    for got in (lp.complex_rank_torch(*args, sides=sides, filter=F, node_type_offsets=offs, chunk=50),
                lp.complex_rank(*args, sides=sides, filter=F, node_type_offsets=offs),
                dec.rank(args[0], *args[2:], sides=sides, filter=F, node_type_offsets=offs)):
        for name, field in (("greater", got.greater), ("equal", got.equal), ("cands", got.candidates)):
            assert field.dtype == torch.int32 and torch.equal(field, torch.tensor(want[name]).to(torch.int32)), name
        assert torch.equal(got.bad, torch.tensor(want["bad"]))
    # the ranks of the two sides differ where the reference says they do, and DistMult's reference cannot tell them apart
    both = ref.rank_reference(h, w, s, r, o, "both")
    P2 = len(s)
    assert (both["greater"][:P2] != both["greater"][P2:]).any()
    m = lp.ranking_metrics(lp.complex_rank_torch(*args, sides="both"))
    assert m["queries"] == 2 * P2 - 6 and 0.0 < m["mrr"] <= 1.0
    with pytest.raises(ValueError, match="sides"):
        lp.complex_rank(*args, sides="left")
    with pytest.raises(ValueError, match="even"):
        lp.complex_rank(torch.zeros(4, 3), torch.zeros(2, 3), *args[2:])
