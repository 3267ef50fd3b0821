"""The ComplEx score kernels (the ComplExTerms instantiations of csrc/triple_score.hip) and the ComplEx head (het_amd/linkpred.py) on
the GPU against the numpy restatement of the rule (tests/_complex_ref.py): the three outputs exactly on integer grids over the ladder
of slot counts around the long-list threshold L, the relation-chunk ladder and every lane-mapping width; normal inputs against fp64
with the staged fp32 emulation as the yardstick; ids outside the tables, bit determinism, uninitialised buffers, the autograd contract,
what the node saves, layouts, the fallback routes, the asymmetry the head exists for, and one training smoke.  Every threshold is read
from kernels.triple_params()."""
import functools

import numpy as np
import pytest
import torch

from tests import _autograd_contract as AC
from tests import _complex_ref as ref
from tests._poison import POISON_IDS, POISONS, poisoned
from tests.util import LADDER, ROW_LADDER, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("fp32", "bf16")


def _k():
    import het_amd.kernels as k
    return k


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bf16_close(got, want, what):
    """The project's bf16 rule: elementwise within 2^-8 |ref| + 1e-5 max|ref|."""
    want = np.asarray(want, dtype=np.float64)
    got = got.detach().float().cpu().double().numpy()
    bound = 2.0 ** -8 * np.abs(want) + 1e-5 * float(np.abs(want).max(initial=0.0))
    worst = float((np.abs(got - want) - bound).max(initial=-1.0))
    assert worst <= 0.0, f"{what}: {worst:.3e} beyond the bf16 bound"


# ---------------------------------------------------------------------------------------------------- the exact structure ladder
def _counts():
    L = _k().triple_long_list()
    return tuple(LADDER) + (L - 1, L, L + 1, 2 * L + 1)


@functools.lru_cache(maxsize=None)
def _ladder_triples(R):
    """(s, r, o, N): node k owns exactly _counts()[k] slots -- head slots, tail slots and self-pairs mixed --, a filler node takes the
    odd stub, three nodes own nothing, and (R > 1) relation 1 owns nothing.  (The construction of tests/test_gpu_triple_score.py.)"""
    counts = _counts()
    rng = np.random.default_rng(200 + R)
    stubs, pairs = [], []
    for k, c in enumerate(counts):
        selfs = min(c // 2, 1 + k % 3)  # a few self-pairs s == o per node that has room for them
        pairs += [(k, k)] * selfs
        stubs += [k] * (c - 2 * selfs)
    filler = len(counts)
    if len(stubs) % 2:
        stubs.append(filler)
    stubs = rng.permutation(stubs)
    pairs += list(zip(stubs[0::2].tolist(), stubs[1::2].tolist()))
    order = rng.permutation(len(pairs))
    s = np.array([pairs[i][0] for i in order], dtype=np.int64)
    o = np.array([pairs[i][1] for i in order], dtype=np.int64)
    r = rng.integers(0, R, len(s))
    if R > 1:
        r[r == 1] = 0
    N = filler + 4  # the filler and three nodes without a triple
    owned = np.bincount(np.concatenate([s, o]), minlength=N)
    assert tuple(owned[:len(counts)]) == counts and not owned[filler + 1:].any() and (s == o).sum() >= len(counts) // 2
    heads, tails = set(s.tolist()), set(o.tolist())
    assert len(heads & tails) > len(counts) // 2  # most nodes own head slots and tail slots: both sides of the node walk
    return s, r, o, N


def _exact_inputs(N, R, T, D, seed):
    """h in -2..2, w in {-1, 0, 1, 2}, g in {+-1, +-2, +-0.5}: exact in fp32 and bf16.  A term of a gradient element is at most
    |g| (|b_r| |x_r| + |b_i| |x_i|) <= 16 and a list has at most 2 T terms; a score is at most 32 per component: every partial sum is
    a multiple of 1/2 far below 2^24, so fp32 is exact in any order."""
    assert 16 * 2 * max(T, 1) < 2 ** 20 and 32 * D < 2 ** 20
    rng = np.random.default_rng(seed)
    grid = lambda values, shape: rng.choice(np.asarray(values, dtype=np.float64), size=shape)  # noqa: E731
    return grid((-2, -1, 0, 1, 2), (N, D)), grid((-1, 0, 1, 2), (R, D)), grid((1, -1, 2, -2, 0.5, -0.5), (T,))


def _run(h, w, s, r, o, g, dtype):
    """(score, grad_h, grad_w, plan) through the wrappers."""
    k = _k()
    hd, wd, gd = _dev(h, dtype), _dev(w, torch.float32), _dev(g, torch.float32)
    sd, rd, od = _dev(s), _dev(r), _dev(o)
    score = k.complex_score(hd, wd, sd, rd, od)
    plan = k.triple_plan(sd, rd, od, h.shape[0], w.shape[0])
    gh, gw = k.complex_score_backward(hd, wd, sd, rd, od, gd, plan)
    assert score.dtype == torch.float32 and score.shape == (len(s),)
    assert gh.dtype == dtype and gh.shape == h.shape and gw.dtype == torch.float32 and gw.shape == w.shape
    return score, gh, gw, plan


def _assert_exact(h, w, s, r, o, g, dtype, what):
    score, gh, gw, plan = _run(h, w, s, r, o, g, dtype)
    want_gh, want_gw = ref.grads(h, w, s, r, o, g)
    assert torch.equal(score.cpu(), torch.tensor(ref.scores(h, w, s, r, o)).float()), what + " score"
    assert torch.equal(gh.cpu(), torch.tensor(want_gh).to(dtype)), what + " grad_h"
    assert torch.equal(gw.cpu(), torch.tensor(want_gw).float()), what + " grad_w"
    return score, gh, gw, plan


def _widths():
    k = _k()
    p = k.triple_params()
    out = {p["min_width"], 8, 64, 128, 256, p["max_width"]}
    for t in k.triple_lane_thresholds():
        out |= {t - 4, t, t + 4}
    return tuple(sorted(d for d in out if k.triple_width_ok(d)))


@pytest.mark.parametrize("R", (1, 5, 91))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_exact_structure_ladder(dtype, R):
    k = _k()
    p = k.triple_params()
    s, r, o, N = _ladder_triples(R)
    L = k.triple_long_list()
    assert {L - 1, L, L + 1, 2 * L + 1} <= set(_counts()) and set(k.triple_lane_thresholds()) <= set(_widths())
    assert {p["min_width"], p["max_width"]} <= set(_widths())
    for D in _widths():
        h, w, g = _exact_inputs(N, R, len(s), D, 7 * D + R)
        _, gh, gw, plan = _assert_exact(h, w, s, r, o, g, dtype, f"R={R} D={D} {dtype}")
        assert not bool(gh[-3:].float().any()) and not bool(torch.signbit(gh[-3:].float()).any())  # nodes without a triple: +0
        if R > 1:
            assert not bool(gw[1].any()) and not bool(torch.signbit(gw[1]).any())  # the relation without a triple: +0
    assert plan.bad.cpu().tolist() == [0]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_exact_relation_chunk_ladder_and_triple_counts(dtype):
    """Relations that own exactly chunk - 1, chunk, chunk + 1 and 2 chunk + 1 triples, and one that owns none; then the row ladder of
    triple counts, T = 0 included."""
    C = _k().triple_params()["rel_chunk"]
    lens = (C - 1, C, 0, C + 1, 2 * C + 1)
    rng = np.random.default_rng(17)
    r = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    N, T = 40, len(r)
    s, o = rng.integers(0, N, T), rng.integers(0, N, T)
    for D in (4, 36):
        h, w, g = _exact_inputs(N, len(lens), T, D, D)
        _, _, gw, plan = _assert_exact(h, w, s, r, o, g, dtype, f"rel chunks D={D} {dtype}")
        assert not bool(gw[2].any())
    assert (plan.rel_ptr[1:] - plan.rel_ptr[:-1]).cpu().tolist() == list(lens)
    for T in ROW_LADDER:
        rng = np.random.default_rng(T)
        s, r, o = rng.integers(0, 50, T), rng.integers(0, 5, T), rng.integers(0, 50, T)
        h, w, g = _exact_inputs(50, 5, T, 64, T + 1)
        _, gh, gw, _ = _assert_exact(h, w, s, r, o, g, dtype, f"T={T} {dtype}")
        if T == 0:  # no triples: both gradients are still written, +0
            assert not bool(gh.float().any()) and not bool(gw.any())


def test_a_triple_and_its_reverse_score_differently_and_the_identities_hold():
    """The property the head exists for, on the kernels: score(s, r, o) != score(o, r, s); with Im(w) = 0 the DistMult kernel's scores
    with each real weight in both columns; with Re(w) = 0 antisymmetry.  Integer grids: exact."""
    k = _k()
    rng = np.random.default_rng(3)
    N, R, T, D = 33, 4, 500, 20
    h, w, _ = _exact_inputs(N, R, T, D, 4)
    s, r, o = rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)
    hd, ids = _dev(h, torch.float32), [_dev(a) for a in (s, r, o)]
    rev = [ids[2], ids[1], ids[0]]
    fwd, bwd = k.complex_score(hd, _dev(w, torch.float32), *ids), k.complex_score(hd, _dev(w, torch.float32), *rev)
    want_f, want_b = ref.scores(h, w, s, r, o), ref.scores(h, w, o, r, s)
    assert torch.equal(fwd.cpu(), torch.tensor(want_f).float()) and torch.equal(bwd.cpu(), torch.tensor(want_b).float())
    assert (want_f != want_b).sum() > T // 2 and int((fwd != bwd).sum()) == int((want_f != want_b).sum())
    assert torch.equal(k.distmult_score(hd, _dev(w, torch.float32), *ids), k.distmult_score(hd, _dev(w, torch.float32), *rev))
    w_re, w_im = w.copy(), w.copy()
    w_re[:, 1::2] = 0
    w_im[:, 0::2] = 0
    both = np.repeat(w[:, 0::2], 2, axis=1)
    assert torch.equal(k.complex_score(hd, _dev(w_re, torch.float32), *ids), k.distmult_score(hd, _dev(both, torch.float32), *ids))
    a, b = k.complex_score(hd, _dev(w_im, torch.float32), *ids), k.complex_score(hd, _dev(w_im, torch.float32), *rev)
    assert torch.equal(a, -b) and bool(a.any())


# ------------------------------------------------------------------------------------------------------------ random normal inputs
def _random_case(N, T, D, seed, dtype, R=5):
    """Normal inputs (bf16: rounded to it first), one hub node of 4 L + 3 slots."""
    L = _k().triple_long_list()
    rng = np.random.default_rng(seed)
    h = torch.tensor(rng.standard_normal((N, D)), dtype=torch.float32).to(dtype).double().numpy()
    w = torch.tensor(rng.standard_normal((R, D)), dtype=torch.float32).double().numpy()
    g = torch.tensor(rng.standard_normal(T), dtype=torch.float32).double().numpy()
    s, r, o = rng.integers(1, N, T), rng.integers(0, R, T), rng.integers(1, N, T)  # node 0 is the hub
    at = rng.permutation(T)[:4 * L + 3]
    o[at[::2]] = 0
    s[at[1::2]] = 0
    assert (s == 0).sum() + (o == 0).sum() == 4 * L + 3
    return h, w, g, s, r, o


@functools.lru_cache(maxsize=None)
def _normal_reference(D, dtype):
    """The case, its fp64 scores and gradients and (fp32) the staged emulation: computed once."""
    p = _k().triple_params()
    h, w, g, s, r, o = _random_case(257, 3001, D, 11 + D, dtype)
    emu = ref.staged_grads(h, w, s, r, o, g, p["list_chunk"], p["rel_chunk"]) if dtype == torch.float32 else None
    return (h, w, g, s, r, o), ref.scores(h, w, s, r, o), ref.grads(h, w, s, r, o, g), emu


@pytest.mark.parametrize("D", (64, 100))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_random_inputs_against_fp64(dtype, D):
    """(N, T, D) = (257, 3001, 64) and (257, 3001, 100), one hub of 4 L + 3 slots.  fp32: scores within tests.util.assert_close of
    fp64; grad_h and grad_w row by row, max_v d_hip[v] <= 2 max_v d_ref[v] with d the relative row error against fp64 and d_ref that
    of the staged fp32 emulation of the kernels' order (tests/_complex_ref.py, never the kernel).  bf16 rows: grad_h elementwise
    within the bf16 bound, grad_w as fp32 (it is summed in fp32).  Measured on an MI355X (printed by this test): DESIGN.md 4.16."""
    from tests._rgat_bf16_train_ref import check_rowwise
    case, want_score, (want_gh, want_gw), emu = _normal_reference(D, dtype)
    h, w, g, s, r, o = case
    score, gh, gw, _ = _run(h, w, s, r, o, g, dtype)
    assert_close(score, torch.tensor(want_score), what=f"D={D} {dtype} score")
    if dtype == torch.float32:
        check_rowwise(f"complex D={D} grad_h", gh, torch.tensor(want_gh), torch.tensor(emu[0]))
        check_rowwise(f"complex D={D} grad_w", gw, torch.tensor(want_gw), torch.tensor(emu[1]))
    else:
        _bf16_close(gh, want_gh, f"D={D} grad_h")
        assert_close(gw, torch.tensor(want_gw), what=f"D={D} {dtype} grad_w")


# -------------------------------------------------------------------------------------------------------------------------- bad ids
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ids_outside_the_tables_are_counted_and_change_nothing_else(dtype):
    from het_amd.linkpred import ComplExDecoder
    N, T, D, R = 257, 1500, 64, 5
    h, w, g, s, r, o = _random_case(N, T, D, 5, dtype, R)
    clean = _run(h, w, s, r, o, g, dtype)
    # four bad triples spliced in: s = -1, o = N, r = R, r = -5
    at = np.array([0, 700, 701, T])
    s2, r2, o2, g2 = (np.insert(a, at, v) for a, v in ((s, [-1, 3, 4, 5]), (r, [0, 1, R, -5]), (o, [2, N, 6, 7]), (g, [9.0, 9.0, 9.0, 9.0])))
    score, gh, gw, plan = _run(h, w, s2, r2, o2, g2, dtype)
    keep = np.ones(T + 4, dtype=bool)
    keep[at + np.arange(4)] = False
    assert plan.bad.cpu().tolist() == [4] and clean[3].bad.cpu().tolist() == [0]
    assert score.cpu()[~keep].tolist() == [0.0] * 4 and not bool(torch.signbit(score.cpu()[~keep]).any())
    assert torch.equal(score.cpu()[keep], clean[0].cpu()) and torch.equal(gh, clean[1]) and torch.equal(gw, clean[2])
    # the module: the count of the last call on the device, with and without a gradient; check_ids raises
    dec = ComplExDecoder(R, D).to(DEV)
    x = _dev(h, dtype)
    ids = [_dev(a) for a in (s2, r2, o2)]
    with torch.no_grad():
        dec(x, *ids)
    assert dec.last_bad.is_cuda and dec.last_bad.tolist() == [4]
    dec(x.clone().requires_grad_(True), *ids)
    assert dec.last_bad.tolist() == [4]
    dec(x, *[_dev(a) for a in (s, r, o)])
    assert dec.last_bad.tolist() == [0]
    with pytest.raises(ValueError, match="4 triple"):
        ComplExDecoder(R, D, check_ids=True).to(DEV)(x, *ids)


# ---------------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_same_bits_on_every_call(dtype):
    h, w, g, s, r, o = _random_case(257, 3001, 64, 21, dtype)
    first = _run(h, w, s, r, o, g, dtype)[:3]
    second = _run(h, w, s, r, o, g, dtype)[:3]
    junk = [torch.randn(n, device=DEV) for n in (1000, 77777, 13)]  # unrelated allocations move every buffer
    other = _random_case(129, 777, 32, 22, dtype)
    _run(*other[:2], *other[3:], other[2], dtype)
    third = _run(h, w, s, r, o, g, dtype)[:3]
    del junk
    for name, a, b, c in zip(("score", "grad_h", "grad_w"), first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c), name


# ------------------------------------------------------------------------------------------------------------ uninitialised buffers
@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_no_result_depends_on_uninitialised_memory(dtype, value):
    from het_amd.linkpred import ComplExDecoder

    def run(case):
        h, w, g, s, r, o = case
        dec = ComplExDecoder(w.shape[0], h.shape[1]).to(DEV)
        with torch.no_grad():
            dec.w_relation.copy_(_dev(w, torch.float32))
        x = _dev(h, dtype).requires_grad_(True)
        score = dec(x, _dev(s), _dev(r), _dev(o))
        score.backward(_dev(g, torch.float32))
        return score.detach().clone(), x.grad.clone(), dec.w_relation.grad.clone(), dec.last_bad.clone()

    s, r, o, N = _ladder_triples(5)
    cases = [_random_case(257, 3001, 64, 31, dtype), _exact_inputs(N, 5, len(s), 36, 32) + (s, r, o)]
    cases[0][3][5] = -1  # (one bad triple)
    for case in cases:
        clean = run(case)
        with poisoned(value) as record:
            dirty = run(case)
        for fn in ("_complex_score", "_complex_score_backward", "_workspace"):
            assert record.from_module("het_amd.kernels", fn), fn
        for name, x, y in zip(("score", "grad_h", "grad_w", "bad"), clean, dirty):
            assert torch.equal(x, y), f"{name} depends on what an unwritten slot held"


# ------------------------------------------------------------------------------------------------------------ the autograd contract
class _Triples:
    """The batch in the place of the layer cases' graph: moved to the device with ``to_``."""

    def __init__(self, s, r, o):
        self.s, self.r, self.o = (torch.tensor(a) for a in (s, r, o))

    def to_(self, dev):
        self.s, self.r, self.o = (t.to(dev) for t in (self.s, self.r, self.o))


def contract_case(dtype, N=61, R=3, T=600, D=32, cols=4):
    """A tests._autograd_contract.Case for ComplExDecoder: the layer is the module, x is h, the output is the scores viewed
    [T / cols, cols] (the clauses hand over two-dimensional gradients in several strides)."""
    from het_amd.linkpred import ComplExDecoder
    rng = np.random.default_rng(3)
    s, r, o = rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)
    o[::9] = s[::9]
    torch.manual_seed(5)
    w0 = ComplExDecoder(R, D).w_relation.detach().clone()

    def make():
        layer = ComplExDecoder(R, D)
        with torch.no_grad():
            layer.w_relation.copy_(w0)
        batch = _Triples(s, r, o)

        def call(x, block=False):
            return layer(x, batch.s, batch.r, batch.o).view(-1, cols)
        call.block_graph = None
        call.operands = lambda: {"s": batch.s, "r": batch.r, "o": batch.o}
        return layer, batch, call

    def inputs(seed, block=False):
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(N, D, generator=gen).to(dtype).float()
        go = torch.randn(T // cols, cols, generator=gen).to(dtype).float()
        return x, go

    cache = {}

    def oracle(calls):
        key = AC.fingerprint(*(t for x, go, _ in calls for t in (x, go)))
        if key not in cache:
            w = w0.double().numpy()
            outs, gxs, gw = [], [], np.zeros_like(w)
            for x, go, _ in calls:
                x64, g64 = x.double().numpy(), go.double().reshape(-1).numpy()
                outs.append(torch.tensor(ref.scores(x64, w, s, r, o)).view(-1, cols))
                gh, gwi = ref.grads(x64, w, s, r, o, g64)
                gxs.append(torch.tensor(gh))
                gw = gw + gwi
            cache[key] = AC.Expected(outs, gxs, {"w_relation": torch.tensor(gw)})
        return cache[key]

    def close(actual, expected, what):
        if actual.dtype == torch.bfloat16:
            _bf16_close(actual, expected.numpy(), what)
        else:
            assert_close(actual, expected, what=what)

    return AC.Case(name=f"complex_{'bf16' if dtype == torch.bfloat16 else 'fp32'}", make=make, leaves=("w_relation",), inputs=inputs,
                   oracle=oracle, close=close, dtype=dtype, frozen=("w_relation",), block=False)


@pytest.mark.parametrize("clause", sorted(AC.CLAUSES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_autograd_contract(dtype, clause, monkeypatch):
    from het_amd import linkpred
    calls = []
    real = linkpred.ComplExScoreFunction.forward
    monkeypatch.setattr(linkpred.ComplExScoreFunction, "forward", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    AC.run_clause(clause, contract_case(dtype), DEV)
    assert calls, "the clause did not run the native node"


def test_double_backward_is_refused_and_other_id_types_are_cast():
    from het_amd.linkpred import ComplExDecoder
    rng = np.random.default_rng(41)
    dec = ComplExDecoder(3, 16).to(DEV)
    x = torch.randn(65, 16, device=DEV, requires_grad=True)
    ids = [_dev(rng.integers(0, n, 300)) for n in (65, 3, 65)]
    score = dec(x, *ids)
    (gx,) = torch.autograd.grad((score * score).sum(), x, create_graph=True)  # (a grad_score that itself requires a gradient)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()
    assert torch.equal(dec(x, *[t.to(torch.int32) for t in ids]), score)
    # a module built with native=False takes the torch composition, which differentiates twice
    slow = ComplExDecoder(3, 16, native=False).to(DEV)
    out = slow(x, *ids)
    (gx,) = torch.autograd.grad((out * out).sum(), x, create_graph=True)
    gx.sum().backward()
    assert slow.w_relation.grad is not None


def test_the_node_saves_nothing_of_t_times_d_elements():
    from het_amd.linkpred import ComplExDecoder
    N, R, T, D = 64, 3, 4096, 64
    rng = np.random.default_rng(0)
    dec = ComplExDecoder(R, D).to(DEV)
    x = torch.randn(N, D, device=DEV, requires_grad=True)
    ids = [_dev(rng.integers(0, n, T)) for n in (N, R, N)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    score = dec(x, *ids)
    torch.cuda.synchronize()
    node = score.grad_fn
    assert "ComplExScoreFunction" in type(node).__name__
    held = list(node.saved_tensors) + list(node.ids) + [t for t in node.plan if isinstance(t, torch.Tensor)]
    assert len(held) >= 11 and max(t.numel() for t in held) < T * D
    assert torch.cuda.memory_allocated() - before < T * D * 4  # what the call keeps alive is below one [T, D] fp32 tensor
    # without a gradient no plan is built
    with torch.no_grad():
        assert dec(x, *ids).grad_fn is None


# ------------------------------------------------------------------------------------------------------------------ layouts, routes
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_strided_and_misaligned_rows_run_on_a_copy(dtype):
    from het_amd.linkpred import ComplExDecoder
    s, r, o, N = _ladder_triples(5)
    D = 36
    h, w, g = _exact_inputs(N, 5, len(s), D, 61)
    want = (torch.tensor(ref.scores(h, w, s, r, o)).float(),) + tuple(torch.tensor(a) for a in ref.grads(h, w, s, r, o, g))
    ids, gd = [_dev(a) for a in (s, r, o)], _dev(g, torch.float32)
    wide = torch.zeros(N, 2 * D, dtype=dtype, device=DEV)
    wide[:, ::2] = _dev(h, dtype)
    flat = torch.zeros(h.size + 1, dtype=dtype, device=DEV)
    flat[1:] = _dev(h, dtype).reshape(-1)
    wflat = torch.zeros(w.size + 1, device=DEV)
    wflat[1:] = _dev(w, torch.float32).reshape(-1)
    for ht, wt in ((wide[:, ::2], _dev(w, torch.float32)), (flat[1:].view(h.shape), _dev(w, torch.float32)),
                   (_dev(h, dtype), wflat[1:].view(w.shape))):
        assert not ht.is_contiguous() or ht.data_ptr() % 16 or wt.data_ptr() % 16
        dec = ComplExDecoder(5, D).to(DEV)
        dec.w_relation = torch.nn.Parameter(wt)
        x = ht.detach().requires_grad_(True)
        assert dec.takes_native(x)
        score = dec(x, *ids)
        score.backward(gd)
        assert torch.equal(score.detach().cpu(), want[0]) and torch.equal(x.grad.cpu(), want[1].to(dtype))
        assert torch.equal(dec.w_relation.grad.cpu(), want[2].float())


def test_fallback_routes_agree_with_the_native_route():
    from het_amd.linkpred import ComplExDecoder
    N, R, T = 257, 5, 3001
    h, w, g, s, r, o = _random_case(N, T, 64, 51, torch.float32, R)
    ids = [_dev(a) for a in (s, r, o)]
    gd = _dev(g, torch.float32)

    def step(dec, x):
        dec.w_relation.grad = None
        x = x.clone().requires_grad_(True)
        score = dec(x, *ids)
        score.backward(gd)
        return score.detach(), x.grad, dec.w_relation.grad.clone()

    dec = ComplExDecoder(R, 64).to(DEV)
    with torch.no_grad():
        dec.w_relation.copy_(_dev(w, torch.float32))
    x32 = _dev(h, torch.float32)
    assert dec.takes_native(x32) and not dec.takes_native(x32.double()) and not dec.takes_native(x32.half()) and not dec.takes_native(x32.cpu())
    native = step(dec, x32)
    wide = step(dec, x32.double())
    dec.native = False
    forced = step(dec, x32)
    dec.native = True
    assert wide[1].dtype == torch.float64 and wide[0].dtype == torch.float32
    for other in (wide, forced):
        for name, a, b in zip(("score", "grad_h", "grad_w"), native, other):
            assert_close(a, b.cpu(), what=name)
    # an even width that is no multiple of 4: the composition, against the reference
    h, w, g, s, r, o = _random_case(N, T, 10, 52, torch.float32, R)
    dec = ComplExDecoder(R, 10).to(DEV)
    with torch.no_grad():
        dec.w_relation.copy_(_dev(w, torch.float32))
    x = _dev(h, torch.float32)
    assert not dec.takes_native(x)
    ids, gd = [_dev(a) for a in (s, r, o)], _dev(g, torch.float32)
    got = step(dec, x)
    want_gh, want_gw = ref.grads(h, w, s, r, o, g)
    assert_close(got[0], torch.tensor(ref.scores(h, w, s, r, o)), what="D=10 score")
    assert_close(got[1], torch.tensor(want_gh), what="D=10 grad_h")
    assert_close(got[2], torch.tensor(want_gw), what="D=10 grad_w")


# ------------------------------------------------------------------------------------------------------------------- training smoke
def test_training_script_complex_decoder_smoke(capsys):
    from het_amd import train
    argv = ["--model", "rgcn", "--link_prediction", "--full_graph_training", "--scale", "0.002", "-e", "3", "--num_layers", "2", "--n_infeat", "64",
            "--num_classes", "64", "--batch_size", "256", "--num_negatives", "2", "--dropout", "0", "--seed", "3", "--decoder", "complex",
            "--eval_ranking", "64"]
    a, b = train.main(argv), train.main(argv)
    capsys.readouterr()
    assert a["task"] == "link_prediction" and a["args"]["decoder"] == "complex" and a["args"]["eval_ranking"] == 64
    assert np.isfinite(a["final_loss"]) and 0.0 < a["final_loss"] < 10.0
    assert np.float32(a["final_loss"]).tobytes() == np.float32(b["final_loss"]).tobytes(), (a["final_loss"], b["final_loss"])
    rk = a["ranking"]
    assert set(rk) == {"mrr", "mean_rank", "hits@1", "hits@3", "hits@10", "queries", "ms"}
    assert rk["queries"] == 128 and 0.0 < rk["mrr"] <= 1.0 and rk["mean_rank"] >= 1.0 and 0.0 <= rk["hits@1"] <= rk["hits@3"] <= rk["hits@10"] <= 1.0
    assert {k: v for k, v in rk.items() if k != "ms"} == {k: v for k, v in b["ranking"].items() if k != "ms"}
    # a default run's log line names no decoder
    plain = train.main(argv[:-4])
    capsys.readouterr()
    assert "decoder" not in plain["args"] and plain["task"] == "link_prediction"
