"""The RGCN layer with block-diagonal relation weights (regularizer="bdd") on the GPU: the per-node row list, the native kernels exact
on integer grids (tests/_rgcn_bdd_ref.py: every partial sum is exact in fp32, so torch.equal against the fp64 reference), normal
inputs at the project's fp32 tolerance, the same bits on two calls, poisoned allocations, the autograd contract, and the calls that
take the dense route.  Every native case asserts layer.last_route and watches the library calls: a silent fallback fails."""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

from tests import _autograd_contract as AC
from tests import _rgcn_bdd_cases as CS
from tests import _rgcn_bdd_ref as REF
from tests._poison import POISON_IDS, POISONS, poisoned
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BDD_ENTRIES = ("het_rgcn_bdd_layer_forward", "het_rgcn_bdd_layer_backward")
DENSE_ENTRIES = ("het_rgcn_layer_forward", "het_rgcn_layer_backward", "het_rgcn_layer1_separate_coo",
                 "het_backward_rgcn_layer1_separate_coo")


def _params():
    import het_amd.kernels as k
    return k.rgcn_bdd_params()


_GPU_GRAPHS = {}


def _gpu_graph(name, arg=0):
    if (name, arg) not in _GPU_GRAPHS:
        g = copy.deepcopy(CS.graph(name, arg))
        g.to_(DEV)
        _GPU_GRAPHS[name, arg] = g
    return _GPU_GRAPHS[name, arg]


@pytest.fixture
def calls(monkeypatch):
    """Names of the library entries called through het_amd._lib.call, counted."""
    from het_amd import _lib
    seen, real = collections.Counter(), _lib.call

    def call(name, *a):
        seen[name] += 1
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def _assert_native(layer, calls, backward=True):
    assert layer.last_route == "native", layer.last_route
    assert calls[BDD_ENTRIES[0]] > 0 and (not backward or calls[BDD_ENTRIES[1]] > 0), dict(calls)
    assert not any(calls[n] for n in DENSE_ENTRIES), dict(calls)


def _layer(R, K, D, B, weight=None, bias=None, has_bias=True):
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    torch.manual_seed(0)
    layer = HET_EglRelGraphConv_EdgeParallel(K, D, R, B, regularizer="bdd", bias=has_bias)
    with torch.no_grad():
        if weight is not None:
            layer.weight.copy_(torch.as_tensor(weight))
        if has_bias:
            layer.h_bias.copy_(torch.as_tensor(bias) if bias is not None else torch.linspace(-0.1, 0.1, D))
    return layer.to(DEV)


def _step(layer, g, x, norm, go, x_grad=True):
    xd = torch.as_tensor(x).to(DEV).requires_grad_(x_grad)
    out = layer(g, xd, torch.as_tensor(norm).to(DEV))
    out.backward(torch.as_tensor(go).to(DEV))
    torch.cuda.synchronize()
    return out.detach(), xd.grad, layer.weight.grad, (layer.h_bias.grad if layer.bias else None)


@functools.lru_cache(maxsize=None)
def _grid_reference(name, arg, shape, seed=7):
    """(case, out, grad_x, grad_w, grad_b) of the grid case on a graph: the fp64 reference, computed once and never changed."""
    K, D, B = shape
    g = CS.graph(name, arg)
    src, dst, rel, eid = CS.coo_of(g)
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    c = REF.grid_case(N, E, R, K, D, B, seed=seed)
    assert REF.grid_units_bound(N, src, dst, rel, eid, c) < 2 ** 24  # (any summation order is exact in fp32)
    out = REF.bdd_forward(N, src, dst, rel, eid, c["norm"], c["x"], c["weight"], c["bias"])
    return (c, out) + REF.bdd_backward(N, src, dst, rel, eid, c["norm"], c["x"], c["weight"], c["go"])


def _equal(name, a, ref):
    a = a.detach().cpu().double().numpy()
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    bad = int((a != ref).sum())
    assert bad == 0, f"{name}: {bad} of {a.size} elements differ from the fp64 reference, max |diff| {np.abs(a - ref).max():.3e}"


def _check_exact(name, arg, shape, calls):
    K, D, B = shape
    c, out, gx, gw, gb = _grid_reference(name, arg, shape)
    g = _gpu_graph(name, arg)
    layer = _layer(g.get_num_rels(), K, D, B, c["weight"], c["bias"])
    o, dx, dw, db = _step(layer, g, c["x"], c["norm"], c["go"])
    _assert_native(layer, calls)
    for what, a, ref in (("out", o, out), ("grad_x", dx, gx), ("grad_weight", dw, gw), ("grad_bias", db, gb)):
        _equal(f"{name} {shape} {what}", a, ref)


# ---------------------------------------------------------------- the per-node row list
@pytest.mark.parametrize("name", ["ladder", "relcount"])
def test_row_list_equals_numpy_and_the_segment_map(name):
    import het_amd.kernels as k
    g = _gpu_graph(name)
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    src, dst, rel, _ = CS.coo_of(CS.graph(name))
    for keys_gpu, payload, keys in ((s["col_indices"], s["row_indices"], dst), (s["row_indices"], s["col_indices"], src)):
        grp = k._plan.get_grouping(s["rel_ptrs"], keys_gpu, N, payload, s["eids"])
        node_ptr, ent_row, ent_rel = (t.cpu().numpy() for t in k.grouping_node_rows(grp, s["rel_ptrs"], keys_gpu, N))
        # numpy: the distinct (relation, key) pairs in (relation, key) order are the grouping's segments; stable sort by key
        pairs = np.unique(rel.numpy() * N + keys.numpy())
        seg_rel, seg_key = pairs // N, pairs % N
        order = np.argsort(seg_key, kind="stable")
        assert np.array_equal(ent_row, order) and np.array_equal(ent_rel, seg_rel[order])
        assert np.array_equal(node_ptr, np.searchsorted(seg_key[order], np.arange(N + 1)))
        # the rows het_grouping_segment_map gives: column n of the [R, N] map, without the -1s, is node n's list
        segmap = k._grouping_segment_map(grp, s["rel_ptrs"], keys_gpu, N).cpu().numpy()
        rr, nn = np.nonzero(segmap.T >= 0)[::-1]
        assert np.array_equal(segmap[rr, nn], ent_row) and np.array_equal(rr, ent_rel)
        assert np.array_equal(np.bincount(nn, minlength=N), np.diff(node_ptr))


# ---------------------------------------------------------------- exact on integer grids
@pytest.mark.parametrize("shape", CS.SHAPES, ids=lambda s: "%dx%db%d" % s)
@pytest.mark.parametrize("name", ["ladder", "relcount"])
def test_exact_on_the_degree_and_relation_count_ladders(name, shape, calls):
    _check_exact(name, 0, shape, calls)


@pytest.mark.parametrize("shape", CS.SHAPES, ids=lambda s: "%dx%db%d" % s)
def test_exact_on_the_rows_per_relation_ladder(shape, calls):
    chunk = _params()["chunk_rows"]
    assert CS.rows_per_relation(CS.graph("rowladder", chunk)).tolist() == list(CS.row_ladder_counts(chunk))
    _check_exact("rowladder", chunk, shape, calls)


def _threshold_cases():
    import het_amd.kernels as k
    out = [("rels", R, (64, 64, 8)) for R in (8, 9, 10)]  # where the dense two-call layer stops
    for K, D, B in CS.SHAPES:  # the LDS weight budget of every shape: the last R held in LDS and the first one beyond
        try:
            r = k.rgcn_bdd_lds_relations(K, D, B)
        except Exception:  # noqa: BLE001 -- collection without a built library: the cases then fail when they run
            r = 1
        out += [("rels", r, (K, D, B)), ("rels", r + 1, (K, D, B))]
    return out


@pytest.mark.parametrize("name,R,shape", _threshold_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_exact_on_both_sides_of_every_relation_count_threshold(name, R, shape, calls):
    import het_amd.kernels as k
    K, D, B = shape
    if R not in (8, 9, 10):  # the last relation count whose blocks fit the LDS budget of this shape, or the first beyond it
        last = k.rgcn_bdd_params()["lds_weight_bytes"] // (4 * K * D // B)
        assert R in (last, last + 1) and last >= 1
    _check_exact(name, R, shape, calls)


# ---------------------------------------------------------------- normal inputs
def _normal_case(name, arg, shape, seed=3):
    K, D, B = shape
    g = CS.graph(name, arg)
    gen = torch.Generator().manual_seed(seed)
    N, E = g.get_num_nodes(), g.get_num_edges()
    return torch.randn(N, K, generator=gen) * 0.5, torch.rand(E, 1, generator=gen), torch.randn(N, D, generator=gen)


@pytest.mark.parametrize("name,shape", [("ladder", (64, 64, 8)), ("ladder", (32, 64, 4)), ("relcount", (128, 128, 4))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_normal_inputs_against_the_reference_and_the_dense_route(name, shape, calls, monkeypatch):
    K, D, B = shape
    x, norm, go = _normal_case(name, 0, shape)
    g = _gpu_graph(name)
    src, dst, rel, eid = CS.coo_of(CS.graph(name))
    N, R = g.get_num_nodes(), g.get_num_rels()
    layer = _layer(R, K, D, B)
    w, b = layer.weight.detach().cpu(), layer.h_bias.detach().cpu()
    ref = (REF.bdd_forward(N, src, dst, rel, eid, norm, x, w, b),) + REF.bdd_backward(N, src, dst, rel, eid, norm, x, w, go)
    native = _step(layer, g, x, norm, go)
    _assert_native(layer, calls)
    names = ("out", "grad_x", "grad_weight", "grad_bias")
    for what, a, r in zip(names, native, ref):
        assert_close(a, torch.from_numpy(r), what=f"native {what}")
    monkeypatch.setenv("HET_RGCN_BDD", "0")
    layer.zero_grad()
    calls.clear()
    dense = _step(layer, g, x, norm, go)
    assert layer.last_route == "dense" and not any(calls[n] for n in BDD_ENTRIES), (layer.last_route, dict(calls))
    for what, a, d, r in zip(names, native, dense, ref):
        assert_close(d, torch.from_numpy(r), what=f"dense {what}")
        assert_close(a, d.cpu().double(), what=f"native against dense {what}")


def test_same_bits_on_two_calls(calls):
    shape = (64, 64, 8)
    x, norm, go = _normal_case("repeat", 0, shape)
    g = _gpu_graph("repeat")
    layer = _layer(g.get_num_rels(), *shape)
    first = [t.clone() for t in _step(layer, g, x, norm, go)]
    layer.zero_grad()
    second = _step(layer, g, x, norm, go)
    _assert_native(layer, calls)
    for what, a, b in zip(("out", "grad_x", "grad_weight", "grad_bias"), first, second):
        assert torch.equal(a, b), what


# ---------------------------------------------------------------- poison
@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
@pytest.mark.parametrize("name", ["relcount", "rowladder"])
def test_exact_under_poisoned_allocations(name, value, calls):
    arg = _params()["chunk_rows"] if name == "rowladder" else 0
    _gpu_graph(name, arg)
    with poisoned(value) as record:
        _check_exact(name, arg, (64, 64, 8), calls)
    assert record.from_module("het_amd.kernels", "rgcn_bdd_layer_forward") and record.from_module("het_amd.kernels", "rgcn_bdd_layer_backward")


# ---------------------------------------------------------------- other calls
def test_num_dst_frozen_leaves_and_an_input_without_gradient(calls):
    shape = (64, 64, 8)
    K, D, B = shape
    c, out, gx, gw, gb = _grid_reference("ladder", 0, shape)
    g = _gpu_graph("ladder")
    R, nd = g.get_num_rels(), 100
    # num_dst: the first rows of the output, gradients of a gradout that is zero beyond them
    layer = _layer(R, K, D, B, c["weight"], c["bias"])
    xd = torch.as_tensor(c["x"]).to(DEV).requires_grad_(True)
    o = layer(g, xd, torch.as_tensor(c["norm"]).to(DEV), num_dst=nd)
    assert tuple(o.shape) == (nd, D)
    _equal("num_dst out", o, out[:nd])
    go = c["go"].copy()
    go[nd:] = 0
    src, dst, rel, eid = CS.coo_of(CS.graph("ladder"))
    rx, rw, rb = REF.bdd_backward(g.get_num_nodes(), src, dst, rel, eid, c["norm"], c["x"], c["weight"], go)
    o.backward(torch.as_tensor(go[:nd]).to(DEV))
    _equal("num_dst grad_x", xd.grad, rx)
    _equal("num_dst grad_weight", layer.weight.grad, rw)
    _equal("num_dst grad_bias", layer.h_bias.grad, rb)
    _assert_native(layer, calls)
    # x needs no gradient: the weight and bias gradients alone
    layer = _layer(R, K, D, B, c["weight"], c["bias"])
    _, dx, dw, db = _step(layer, g, c["x"], c["norm"], c["go"], x_grad=False)
    assert dx is None
    _equal("no grad_x: grad_weight", dw, gw)
    _equal("no grad_x: grad_bias", db, gb)
    # a frozen weight, a frozen bias, no bias at all
    for frozen in ("weight", "h_bias"):
        layer = _layer(R, K, D, B, c["weight"], c["bias"])
        getattr(layer, frozen).requires_grad_(False)
        _, dx, dw, db = _step(layer, g, c["x"], c["norm"], c["go"])
        _equal(f"frozen {frozen}: grad_x", dx, gx)
        assert (dw is None) == (frozen == "weight") and (db is None) == (frozen == "h_bias")
    layer = _layer(R, K, D, B, c["weight"], has_bias=False)
    o, dx, dw, _ = _step(layer, g, c["x"], c["norm"], c["go"])
    _equal("no bias: out", o, out - c["bias"].astype(np.float64)[None, :])
    _equal("no bias: grad_weight", dw, gw)
    _assert_native(layer, calls)


# ---------------------------------------------------------------- the autograd contract
def _contract_case():
    shape = (64, 64, 8)
    K, D, B = shape
    name = "ladder"
    src, dst, rel, eid = CS.coo_of(CS.graph(name))
    g0 = CS.graph(name)
    N, R, E = g0.get_num_nodes(), g0.get_num_rels(), g0.get_num_edges()
    torch.manual_seed(7)
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    proto = HET_EglRelGraphConv_EdgeParallel(K, D, R, B, regularizer="bdd")
    with torch.no_grad():
        proto.h_bias.uniform_(-0.1, 0.1)
    state = {n: t.detach().clone() for n, t in proto.state_dict().items()}
    norm = torch.rand(E, 1, generator=torch.Generator().manual_seed(5))

    def make():
        g = copy.deepcopy(g0)
        layer = HET_EglRelGraphConv_EdgeParallel(K, D, R, B, regularizer="bdd")
        layer.load_state_dict(state)
        norms = {}

        def norm_on():
            dev = g.get_device()
            if dev not in norms:
                norms[dev] = norm.to(dev)
            return norms[dev]

        def call(x, block=False):
            out = layer(g, x, norm_on())
            if x.is_cuda and x.dtype == torch.float32:
                assert layer.last_route == "native", layer.last_route
            return out

        def operands():
            return {"norm": norm_on(), **{"coo_" + k: v for k, v in g.get_separate_coo_original().items()}}
        call.block_graph, call.operands = None, operands
        return layer, g, call

    @functools.lru_cache(maxsize=None)
    def inputs(seed, block=False):
        gen = torch.Generator().manual_seed(1000 * seed)
        return torch.randn(N, K, generator=gen) * 0.5, torch.randn(N, D, generator=gen)

    def oracle(calls_):
        outs, gxs, gw, gb = [], [], 0.0, 0.0
        for x, go, _ in calls_:
            outs.append(torch.from_numpy(REF.bdd_forward(N, src, dst, rel, eid, norm, x, state["weight"], state["h_bias"])))
            rx, rw, rb = REF.bdd_backward(N, src, dst, rel, eid, norm, x, state["weight"], go)
            gxs.append(torch.from_numpy(rx))
            gw, gb = gw + rw, gb + rb
        return AC.Expected(outs, gxs, {"weight": torch.from_numpy(gw), "h_bias": torch.from_numpy(gb)})

    return AC.Case(name="rgcn_bdd", make=make, leaves=("weight", "h_bias"), inputs=inputs, oracle=oracle,
                   close=lambda a, e, what: assert_close(a, e, what=what), frozen=("h_bias",), block=False)


@pytest.mark.parametrize("clause", list(AC.CLAUSES))
def test_autograd_contract(clause, calls):
    AC.run_clause(clause, _contract_case(), DEV)
    assert calls[BDD_ENTRIES[0]] > 0 and calls[BDD_ENTRIES[1]] > 0 and not any(calls[n] for n in DENSE_ENTRIES), dict(calls)


# ---------------------------------------------------------------- calls that take the dense route
def test_a_bf16_input_and_a_one_shot_block_take_the_dense_route(calls):
    from het_amd import sampling
    from tests.test_gpu_rgcn_bf16 import _check_bf16, _check_f32
    shape = (64, 64, 8)
    K, D, B = shape
    x, norm, go = _normal_case("ladder", 0, shape)
    g = _gpu_graph("ladder")
    src, dst, rel, eid = CS.coo_of(CS.graph("ladder"))
    N, R = g.get_num_nodes(), g.get_num_rels()
    layer = _layer(R, K, D, B)
    w, b = layer.weight.detach().cpu(), layer.h_bias.detach().cpu()
    # bf16: the existing layer's behaviour on the dense expansion, held to the bound its bf16 tests use (on the rounded inputs)
    xb, gob = x.to(torch.bfloat16), go.to(torch.bfloat16)
    ref = (REF.bdd_forward(N, src, dst, rel, eid, norm, xb.float(), w, b),) + REF.bdd_backward(N, src, dst, rel, eid, norm, xb.float(), w, gob.float())
    o, dx, dw, db = _step(layer, g, xb, norm, gob)
    assert layer.last_route == "dense" and not any(calls[n] for n in BDD_ENTRIES), (layer.last_route, dict(calls))
    _check_bf16("bf16 out", o.cpu(), torch.from_numpy(ref[0]))
    _check_bf16("bf16 grad_x", dx.cpu(), torch.from_numpy(ref[1]))
    _check_f32("bf16 grad_weight", dw.cpu(), torch.from_numpy(ref[2]))  # (fp32 sums of exactly widened rows)
    _check_f32("bf16 grad_bias", db.cpu(), torch.from_numpy(ref[3]))
    # a one-shot block: groupings off for the step
    ref = (REF.bdd_forward(N, src, dst, rel, eid, norm, x, w, b),) + REF.bdd_backward(N, src, dst, rel, eid, norm, x, w, go)
    layer.zero_grad()
    with sampling.one_shot_graphs():
        got = _step(layer, g, x, norm, go)
    assert layer.last_route == "dense" and not any(calls[n] for n in BDD_ENTRIES), (layer.last_route, dict(calls))
    for what, a, r in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, ref):
        assert_close(a, torch.from_numpy(r), what=f"one-shot {what}")
