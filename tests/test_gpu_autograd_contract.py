"""The autograd contract (tests/_autograd_contract.py: C1 - C8) on every autograd node of the layers, and the grad-mode
rules I1 - I3 that go with C8.  One Case per row of CASES; every case names the node classes and the telling kernel calls of the
route it expects and asserts, after the clause has run, that this is what ran.

Graphs: RGAT and HGT on tests.util.ladder_graph (about 12 700 edges, hubs above 256 in-edges with their hub records and parked
partial sums, an empty relation, isolated nodes, shuffled eids), the block half of C6 on the block a NeighborSampler makes of its first
120 nodes; RGCN on random_graph(seed=41, n=400, r=4, e=6000).  Widths K = 64, X = 64, H = 4 unless the row says otherwise.
hgt_fused, hgt_use_norm and hgt_bf16 run on ladder_graph(R=3): with the five relations of R=5 leaving the graph's one node type the
node-major input gradient is outside its shapes (11 sources per launch) and hgt_route answers per_relation -- which is the row
hgt_per_relation.

Tolerances are the project's own: tests.util.assert_close for fp32; for bf16 the bounds of the existing reference modules as they
stand -- RGCN: _check_bf16 / _check_f32 of tests/test_gpu_rgcn_bf16.py; RGAT and HGT: d_hip <= max(2 d_ref, 1e-5) against the staged
emulations of tests/_rgat_bf16_train_ref.py (with its row-wise criterion for the bf16 rows) and tests/_hgt_bf16_ref.py /
tests/_hgt_use_norm_ref.py, evaluated for exactly the calls the clause made (several calls in one autograd graph included)."""
import collections
import copy
import dataclasses
import functools
from typing import Callable, Optional, Tuple

import pytest
import torch

from oracle import layers as OL
from tests import _autograd_contract as AC
from tests.util import assert_close, ladder_graph, random_graph, rgat_min_abs_preactivation

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
ND = 120  # the destinations of the sampled block: the graph's first 120 nodes (on the ladder graph every destination rung)


@dataclasses.dataclass
class Ref:
    """The fp64 oracle and the staged bf16 emulation of one quantity: what the bf16 criterion d_hip <= max(2 d_ref, 1e-5) needs."""
    ref: torch.Tensor
    emu: torch.Tensor

    def __add__(self, other):  # (fp32 parameter gradients of two backward calls: autograd adds them in fp32, nothing is rounded)
        return Ref(self.ref + other.ref, self.emu + other.emu)


@dataclasses.dataclass
class Spec:
    name: str
    model: str                                  # rgat | rgcn | hgt
    graph: str                                  # ladder5 | ladder3 | rgcn
    layer: Callable                             # (R, T) -> layer on the CPU (seeded by the caller)
    dtype: torch.dtype = torch.float32
    patches: Tuple = ()                         # (module path, attribute, value) set for the duration of the test
    nodes: Tuple[str, ...] = ()                 # autograd Function classes whose forward must run ("module:Class")
    no_nodes: Tuple[str, ...] = ()              # ... and must not
    kernels: Tuple[str, ...] = ()               # het_amd.kernels functions that must be called in a step with a backward
    no_kernels: Tuple[str, ...] = ()            # ... and must not
    route: Optional[Callable] = None            # predicate on the route record of every full-graph call that needs a gradient
    block: bool = True
    K: int = 64
    X: int = 64
    H: int = 4
    emulated: bool = False                      # bf16 RGAT / HGT: expected values are Ref(oracle, emulation)
    use_norm: bool = False


# ---------------------------------------------------------------- graphs, blocks, parameters: built once, never changed
def _new_graph(key):
    return random_graph(seed=41, n=400, r=4, e=6000) if key == "rgcn" else ladder_graph(R=int(key[-1]))


@functools.lru_cache(maxsize=None)
def _graphs(key, by_type):
    """(graph, block graph, global edge id of every block edge) on the CPU."""
    from het_amd.sampling import NeighborSampler
    g = _new_graph(key)
    nd = ND
    sampler = NeighborSampler(g, [-1], by_type=by_type)
    b = sampler.sample_blocks(torch.arange(nd))[0] if by_type else sampler.sample_block(torch.arange(nd), -1)
    assert b.num_dst == nd and torch.equal(b.nodes[:nd], torch.arange(nd))
    return g, b.graph, b.edge_ids


@dataclasses.dataclass
class GraphTensors:
    rp: torch.Tensor
    row: torch.Tensor
    col: torch.Tensor
    eids: torch.Tensor
    N: int
    nd: int
    offs: torch.Tensor
    seg: Optional[torch.Tensor]
    st: torch.Tensor


def _tensors(g, nd):
    s = g.get_separate_coo_original()
    try:
        st = g.get_rel_node_types()[0]
    except ValueError:
        st = None
    return GraphTensors(s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"], g.get_num_nodes(), nd,
                        g.get_original_node_type_offsets(), g.graph_data["original"].get("node_segment_types"), st)


@functools.lru_cache(maxsize=None)
def _state(name):
    """Per case, on the CPU: the graphs' tensors, the layer's parameters and (RGCN) the edge norm."""
    spec = SPECS[name]
    g, blk, edge_ids = _graphs(spec.graph, spec.model == "hgt")
    torch.manual_seed(7)
    layer = spec.layer(g.get_num_rels(), g.get_num_ntypes())
    with torch.no_grad():
        if spec.model == "hgt":
            layer.relation_pri.uniform_(0.5, 1.5)
            layer.skip.uniform_(-1, 1)
            if spec.use_norm:
                layer.norm_weight.uniform_(0.5, 1.5)
                layer.norm_bias.uniform_(-1, 1)
        else:
            layer.h_bias.uniform_(-0.1, 0.1)
    norm = torch.rand(g.get_num_edges(), 1, generator=torch.Generator().manual_seed(5)) if spec.model == "rgcn" else None
    full, block = _tensors(g, g.get_num_nodes()), _tensors(blk, ND)
    return dict(state={n: t.detach().clone() for n, t in layer.state_dict().items()}, full=full, block=block, norm=norm,
                norm_block=None if norm is None else norm[edge_ids], leaves=tuple(n for n, _ in layer.named_parameters()))


# ---------------------------------------------------------------- the fp64 oracle (and the staged bf16 emulation) of one call
def _forward64(spec, p, x, gt, norm, emulate):
    if spec.model == "rgat":
        if emulate:
            from tests import _rgat_bf16_ref as REF
            from tests import _rgat_bf16_train_ref as TREF
            from tests._hgt_bf16_ref import _Round
            with TREF._straight_through_rounding():
                return REF.staged_reference(_Round.apply(x, False, True), p["conv_weights"], p["attn_l"], p["attn_r"], gt.rp, gt.row, gt.col,
                                            gt.N, 0.2, p.get("loop_weight"), p.get("h_bias"), gt.nd, True)
        return OL.rgat_layer(x, p["conv_weights"], p["attn_l"], p["attn_r"], gt.rp, gt.row, gt.col, gt.N, 0.2, p.get("loop_weight"),
                             p.get("h_bias"))[:gt.nd]
    if spec.model == "rgcn":
        return OL.rgcn_layer(x, p["weight"], norm.double()[gt.eids], gt.rp, gt.row, gt.col, gt.N, p["h_bias"])[:gt.nd]
    from tests._hgt_bf16_ref import PARAMS, _Round, staged_emulation
    from tests._typed_layer_norm_ref import typed_layer_norm_ref
    sel = (lambda w: w) if gt.seg is None else (lambda w: w.index_select(0, gt.seg))  # a block: one weight per run of equal type
    if emulate and gt.seg is not None:
        # a bf16 call on a block is served by the upcast route (hgt_route: NATIVE needs a full graph): the fp32 layer on h.float(),
        # the output rounded once and, through autograd's casts, the input gradient rounded once -- the situation of
        # tests/_hgt_bf16_ref.py::check_bf16, which tests/test_gpu_hgt_bf16.py holds that route to.  Its emulation is the oracle with
        # those two roundings; the fp32 parameter gradients pass through unrounded.
        assert not spec.use_norm
        y = OL.hgt_layer(_Round.apply(x, False, True), gt.offs, gt.rp, gt.row, gt.col, gt.N, sel(p["k_linears"]), sel(p["q_linears"]),
                         sel(p["v_linears"]), sel(p["a_linears"]), p["relation_att"], p["relation_msg"], p["relation_pri"], sel(p["skip"]),
                         spec.H, fused_attn=False)
        return _Round.apply(y, True, False)[:gt.nd]
    if emulate:
        y = staged_emulation(x, gt.offs, gt.rp, gt.row, gt.col, gt.N, gt.st, {n: p[n] for n in PARAMS}, spec.H, False, True)
    else:
        y = OL.hgt_layer(x, gt.offs, gt.rp, gt.row, gt.col, gt.N, sel(p["k_linears"]), sel(p["q_linears"]), sel(p["v_linears"]),
                         sel(p["a_linears"]), p["relation_att"], p["relation_msg"], p["relation_pri"], sel(p["skip"]), spec.H, fused_attn=False)
    if spec.use_norm:
        if emulate:
            y = _Round.apply(y, False, True)
        y = typed_layer_norm_ref(y, gt.offs, sel(p["norm_weight"]), sel(p["norm_bias"]), 1e-5)[0]
        if emulate:
            y = _Round.apply(y, True, False)
    return y[:gt.nd]


_ORACLES = {}


def _oracle(name, calls):
    spec, st = SPECS[name], _state(name)
    key = (name, AC.fingerprint(*(t for x, go, _ in calls for t in (x, go))), tuple(bool(b) for _, _, b in calls))
    if key in _ORACLES:
        return _ORACLES[key]

    def run(emulate):
        p = {n: st["state"][n].detach().double().requires_grad_(True) for n in st["leaves"]}
        xs = [x.double().requires_grad_(True) for x, _, _ in calls]
        outs = [_forward64(spec, p, x, st["block" if blk else "full"], st["norm_block" if blk else "norm"], emulate)
                for x, (_, _, blk) in zip(xs, calls)]
        total = sum((o * go.double()).sum() for o, (_, go, _) in zip(outs, calls))
        leaves = xs + [p[n] for n in st["leaves"]]
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(torch.autograd.grad(total, leaves, allow_unused=True), leaves)]
        return [o.detach() for o in outs], grads[:len(xs)], dict(zip(st["leaves"], grads[len(xs):]))

    ref = run(False)
    if spec.emulated:
        emu = run(True)
        pair = lambda r, e: Ref(r, e)  # noqa: E731
        exp = AC.Expected([pair(r, e) for r, e in zip(ref[0], emu[0])], [pair(r, e) for r, e in zip(ref[1], emu[1])],
                          {n: pair(ref[2][n], emu[2][n]) for n in ref[2]})
    else:
        exp = AC.Expected(*ref)
    _ORACLES[key] = exp
    return exp


@functools.lru_cache(maxsize=None)
def _inputs(name, seed, block=False):
    """(x, go) fp32 on the CPU, values the case's dtype holds exactly; RGAT: no (edge, head) pre-activation on the leaky-ReLU kink
    (tests/util.py: rgat_min_abs_preactivation), as every RGAT layer test arranges."""
    spec, st = SPECS[name], _state(name)
    gt = st["block" if block else "full"]
    gen = torch.Generator().manual_seed(1000 * seed + 17 * block)
    rnd = (lambda t: t.to(spec.dtype).float())
    x = rnd(torch.randn(gt.N, spec.K, generator=gen) * 0.5)
    go = rnd(torch.randn(gt.nd, spec.X, generator=gen))
    if spec.model == "rgat":
        s = {"rel_ptrs": gt.rp, "row_indices": gt.row, "col_indices": gt.col}
        W, al, ar = (st["state"][n] for n in ("conv_weights", "attn_l", "attn_r"))
        for _ in range(64):
            if rgat_min_abs_preactivation(x, W, al, ar, s) >= 2e-6:
                break
            x = rnd(x + 1e-3 * torch.randn(gt.N, spec.K, generator=gen))
        else:
            raise AssertionError("no input off the leaky-ReLU kink")
    return x, go


# ---------------------------------------------------------------- tolerances: the project's own
def _rel(a, ref):
    return float((a.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _close(spec):
    if spec.dtype == torch.float32:
        return lambda a, e, what: assert_close(a, e, what=what)
    if spec.model == "rgcn":
        from tests.test_gpu_rgcn_bf16 import _check_bf16, _check_f32

        def close(a, e, what):
            (_check_bf16 if a.dtype == BF16 else _check_f32)(what, a.detach().cpu(), e)
        return close

    def close(a, e, what):
        d_ref, d_hip = _rel(e.emu, e.ref), _rel(a, e.ref)
        print(f"{what}: d_ref {d_ref:.3e} d_hip {d_hip:.3e}")
        assert d_hip <= max(2 * d_ref, 1e-5), f"{what}: d_hip {d_hip:.3e} against d_ref {d_ref:.3e}"
        if spec.model == "rgat" and a.dtype == BF16 and a.dim() == 2:
            from tests._rgat_bf16_train_ref import check_rowwise
            check_rowwise(what, a, e.ref, e.emu)
    return close


# ---------------------------------------------------------------- the Case of a row
def _case(name):
    spec, st = SPECS[name], _state(name)

    def make():
        g, blk, _ = (copy.deepcopy(t) for t in _graphs(spec.graph, spec.model == "hgt"))
        layer = spec.layer(g.get_num_rels(), g.get_num_ntypes())
        layer.load_state_dict(st["state"])
        norms = {}

        def norm_on(which):
            dev = g.get_device()
            if (which, dev) not in norms:
                norms[which, dev] = st[which].to(dev)
            return norms[which, dev]

        def call(x, block=False):
            graph, nd = (blk, {"num_dst": st["block"].nd}) if block else (g, {})
            if spec.model == "rgcn":
                return layer(graph, x, norm_on("norm_block" if block else "norm"), **nd)
            return layer(graph, x, **nd)

        def operands():
            watched = {"coo_" + k: v for k, v in g.get_separate_coo_original().items()}
            if spec.model == "rgcn":
                watched["norm"] = norm_on("norm")
                norm_on("norm_block")
            return watched
        call.block_graph, call.operands = (blk if spec.block else None), operands
        return layer, g, call

    frozen = {"rgat": ("attn_l", "attn_r"), "hgt": ("relation_pri", "relation_att"), "rgcn": ("h_bias",)}[spec.model]
    return AC.Case(name=name, make=make, leaves=st["leaves"], inputs=functools.partial(_inputs, name),
                   oracle=functools.partial(_oracle, name), close=_close(spec), dtype=spec.dtype, frozen=frozen, block=spec.block)


# ---------------------------------------------------------------- the rows
def _rgat(X=64, **kw):
    def build(R, T):
        from het_amd.layers import HET_RGATLayer
        return HET_RGATLayer(64, X, R, 4, bias=True, self_loop=True, dropout=0.0, **kw)
    return build


def _rgcn(K=64, D=64, **kw):
    def build(R, T):
        from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
        return HET_EglRelGraphConv_EdgeParallel(K, D, R, bias=True, **kw)
    return build


def _hgt(**kw):
    def build(R, T):
        from het_amd.layers import HET_HGTLayerHetero
        return HET_HGTLayerHetero(T, R, 64, 64, num_heads=4, dropout=0.0, **kw)
    return build


FL, HF, RB = "het_amd.backend.rgat_fused_layer", "het_amd.backend.hgt_fused_layer", "het_amd.backend.rgcn_layers_and_funcs"
COMPACT = dict(compact_as_of_node_flag=True, compact_direct_indexing_flag=True, multiply_among_weights_first_flag=True)
NODE = FL + ":RgatLayerFunction"
_node_route = lambda r: r.path == "node" and r.compact and r.mulfirst  # noqa: E731
_hgt_route = lambda dx, **kw: (lambda r: r.path == "fused" and r.dx == dx and all(getattr(r, k) == v for k, v in kw.items()))  # noqa: E731
SPECS = {s.name: s for s in (
    Spec("rgat_node_major", "rgat", "ladder5", _rgat(**COMPACT), patches=((FL, "OVERLAP", True),), nodes=(NODE,), route=_node_route,
         kernels=("rgat_node_backward_dx",), no_kernels=("matmul_backward[distinct_rows]",)),
    Spec("rgat_node_major_one_stream", "rgat", "ladder5", _rgat(**COMPACT), patches=((FL, "OVERLAP", False),), nodes=(NODE,),
         route=_node_route, kernels=("rgat_node_backward_dx",), no_kernels=("matmul_backward[distinct_rows]",)),
    Spec("rgat_generic", "rgat", "ladder5", _rgat(X=128, **COMPACT), X=128, nodes=(NODE,), route=_node_route,
         kernels=("matmul_backward[distinct_rows]",), no_kernels=("rgat_node_backward_dx",)),
    Spec("rgat_per_edge", "rgat", "ladder5", _rgat(), patches=((FL, "PER_EDGE", True),), nodes=(NODE,),
         route=lambda r: r.path == "node" and not r.compact, kernels=("fused_gat_forward", "fused_gat_backward"),
         no_kernels=("rgat_backward_compact",)),
    Spec("rgat_composition", "rgat", "ladder5", _rgat(), patches=((FL, "rgat_layer_fused_ok", lambda *a, **k: False),), no_nodes=(NODE,),
         route=lambda r: r.path == "composition", kernels=("fused_gat_forward", "fused_gat_backward")),
    Spec("rgat_bf16_train", "rgat", "ladder5", _rgat(bf16_training=True), dtype=BF16, emulated=True, nodes=(FL + ":RgatLayerBf16Function",),
         no_nodes=(NODE,), route=lambda r: r.path == "train_bf16", kernels=("rgat_node_backward_dx_bf16",)),
    Spec("rgcn_fused", "rgcn", "rgcn", _rgcn(), nodes=(RB + ":RgcnLayerFused",), kernels=("rgcn_layer_forward", "rgcn_layer_backward")),
    Spec("rgcn_fused_bf16", "rgcn", "rgcn", _rgcn(), dtype=BF16, nodes=(RB + ":RgcnLayerFused",),
         kernels=("rgcn_layer_forward_bf16", "rgcn_layer_backward_bf16"), no_kernels=("rgcn_layer_forward",)),
    Spec("rgcn_layer1", "rgcn", "rgcn", _rgcn(16, 16), K=16, X=16, patches=(("het_amd.layers", "PAD_WIDTHS", False),),
         nodes=(RB + ":RgcnLayer1SeparateCooBias",), no_nodes=(RB + ":RgcnLayerFused",)),
    Spec("rgcn_compact", "rgcn", "rgcn", _rgcn(compact_as_of_node_flag=True), nodes=(RB + ":_RGCNCompactAgg",),
         no_nodes=(RB + ":RgcnLayerFused",)),
    Spec("hgt_fused", "hgt", "ladder3", _hgt(), patches=((HF, "COMPACT_DST_BELOW", 2.0),), nodes=(HF + ":HgtAttentionFunction",),
         route=_hgt_route("node_major", compact_dst=True), kernels=("node_rows_matmul_sum", "hgt_backward_compact")),
    Spec("hgt_per_relation", "hgt", "ladder5", _hgt(), nodes=(HF + ":HgtAttentionFunction",), route=_hgt_route("per_relation"),
         kernels=("hgt_backward_compact",), no_kernels=("node_rows_matmul_sum",)),
    Spec("hgt_composition", "hgt", "ladder5", _hgt(), patches=((HF, "FUSED", False),), no_nodes=(HF + ":HgtAttentionFunction",),
         route=lambda r: r.path == "composition"),
    Spec("hgt_use_norm", "hgt", "ladder3", _hgt(use_norm=True), use_norm=True,
         nodes=(HF + ":HgtAttentionFunction", HF + ":TypedLayerNormFunction"), route=_hgt_route("node_major"),
         kernels=("rows_layer_norm", "rows_layer_norm_backward")),
    # (the block half of C6: a native bf16 call alive beside an upcast call of the same layer on the block -- _forward64 has the
    #  emulation of either)
    Spec("hgt_bf16", "hgt", "ladder3", _hgt(), dtype=BF16, emulated=True, nodes=(HF + ":HgtAttentionFunction",),
         route=_hgt_route("node_major", native_bf16=True), kernels=("hgt_backward_compact_bf16", "node_rows_matmul_sum_bf16")),
)}
CASES = list(SPECS)

VARIANTS = (["C1", "C2"] + [f"C3-{x}-{g}" for x, g in AC.C3_FORMS] + ["C4-" + s for s in "abcd"] + ["C5", "C6", "C6-block", "C7"]
            + ["C8-" + m for m in AC.GRAD_MODES])


# ---------------------------------------------------------------- what ran
def _resolve(path):
    import importlib
    mod, _, attr = path.partition(":")
    return getattr(importlib.import_module(mod), attr)


def _watch(spec, monkeypatch):
    """Apply the case's patches; count the forwards of the named autograd nodes, the calls of the named kernels.py functions and
    record every route the two routed layers decide."""
    import importlib

    import het_amd.kernels as k
    from het_amd.layers import HET_HGTLayerHetero, HET_RGATLayer
    for mod, attr, value in spec.patches:
        monkeypatch.setattr(importlib.import_module(mod), attr, value)
    calls, routes = collections.Counter(), []
    for path in spec.nodes + spec.no_nodes:
        cls = _resolve(path)
        real = cls.forward

        def forward(*a, _real=real, _path=path, **kw):
            calls[_path] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(cls, "forward", staticmethod(forward))
    for name in spec.kernels + spec.no_kernels:
        fn, _, flag = name.partition("[")
        real = getattr(k, fn)

        def kernel(*a, _real=real, _name=name, _flag=flag.rstrip("]"), **kw):
            calls[_name] += bool(kw.get(_flag)) if _flag else 1
            return _real(*a, **kw)
        monkeypatch.setattr(k, fn, kernel)
    rgat_route, hgt_route = HET_RGATLayer._route, HET_HGTLayerHetero._route
    trains = lambda layer, x: torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in layer.parameters()))  # noqa: E731

    def rgat(self, g, x, num_dst, halo):
        r = rgat_route(self, g, x, num_dst, halo)
        routes.append((r, num_dst is None and trains(self, x)))  # (the routes of full-graph training calls are what a row names)
        return r

    def hgt(self, G, h, offs):
        r = hgt_route(self, G, h, offs)
        routes.append((r, G.graph_data["original"].get("node_segment_types") is None and trains(self, h)))
        return r
    monkeypatch.setattr(HET_RGATLayer, "_route", rgat)
    monkeypatch.setattr(HET_HGTLayerHetero, "_route", hgt)
    return calls, routes


def _assert_route(spec, calls, routes, backward=True):
    for path in spec.nodes if backward else ():  # (a call that needs no gradient may be served without the node: the evaluation paths)
        assert calls[path] > 0, f"{spec.name}: the node {path} did not run: {dict(calls)}"
    for path in spec.no_nodes:
        assert calls[path] == 0, f"{spec.name}: the node {path} ran: {dict(calls)}"
    if backward:
        for name in spec.kernels:
            assert calls[name] > 0, f"{spec.name}: {name} was not called: {dict(calls)}"
    for name in spec.no_kernels:
        assert calls[name] == 0, f"{spec.name}: {name} was called: {dict(calls)}"
    if spec.route is not None:
        train = [r for r, t in routes if t and r.path != "upcast"]
        assert (train or not backward) and all(spec.route(r) for r in train), f"{spec.name}: routes {train}"


@pytest.mark.parametrize("name,variant", [(n, v) for n in CASES for v in VARIANTS if v != "C6-block" or SPECS[n].block])
def test_contract(name, variant, monkeypatch):
    spec = SPECS[name]
    clause, _, arg = variant.partition("-")
    calls, routes = _watch(spec, monkeypatch)
    case = _case(name)
    if clause == "C3":
        AC.c3_strides(case, DEV, *arg.split("-"))
    elif clause == "C4":
        AC.c4_frozen_leaves(case, DEV, arg)
    elif clause == "C6":
        AC.c6_interleaved_calls(case, DEV, block=arg == "block")
    elif clause == "C8":
        # (state that outlives a graph -- the cached [0, nd] lists of the self-loop -- may have been built by an earlier test in normal
        #  mode: emptied, so that this call builds it inside the mode whatever ran before)
        from het_amd.backend import rgat_fused_layer
        monkeypatch.setattr(rgat_fused_layer, "_OFFS", {})
        AC.c8_evaluate_then_train(case, DEV, arg)
    else:
        AC.CLAUSES[clause](case, DEV)
    _assert_route(spec, calls, routes, backward=variant != "C4-d")


# ---------------------------------------------------------------- I2: a graph made inside inference mode serves evaluation only
I_CASES = ["rgat_node_major", "rgat_per_edge", "rgcn_fused", "hgt_fused", "hgt_use_norm"]


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("name", I_CASES)
def test_i2_a_graph_made_in_inference_mode_evaluates_and_refuses_to_train(name, block, monkeypatch):
    """The graph -- for ``block`` the sampler and its block too -- is built and moved to the device inside torch.inference_mode():
    evaluation there is the oracle's; a call that needs a gradient raises HetError at the layer's entry, before any launch, and the
    message says that the graph's tensors were created in inference mode."""
    import het_amd.kernels as k
    from het_amd._lib import HetError
    from het_amd.sampling import NeighborSampler
    spec, st = SPECS[name], _state(name)
    _watch(spec, monkeypatch)
    case = _case(name)
    x, go = case.inputs(2, block)
    layer = spec.layer(st["full"].rp.numel() - 1, st["full"].offs.numel() - 1)
    layer.load_state_dict(st["state"])
    layer.to(DEV)
    extra = {}
    with torch.inference_mode():
        g = _new_graph(spec.graph)
        g.to_(DEV)
        graph = g
        if block:
            sampler = NeighborSampler(g, [-1], by_type=spec.model == "hgt")
            nd = st["block"].nd
            seeds = torch.arange(nd, device=DEV)
            b = sampler.sample_blocks(seeds)[0] if spec.model == "hgt" else sampler.sample_block(seeds, -1)
            graph, extra = b.graph, {"num_dst": nd}
        args = ()
        if spec.model == "rgcn":
            norm = st["norm"].to(DEV)
            args = (norm[b.edge_ids] if block else norm,)
        out = layer(graph, x.to(DEV), *args, **extra)
        torch.cuda.synchronize()
    assert graph.holds_inference_tensors()
    exp = case.oracle(((x, go, block),))
    case.close(out, exp.outs[0], f"I2 {name} evaluation")
    launches = []
    monkeypatch.setattr(k, "_call", lambda *a, **kw: launches.append(a[1]))
    monkeypatch.setattr(k._lib, "call", lambda *a, **kw: launches.append(a[0]))
    with pytest.raises(HetError, match="created in inference mode"):
        layer(graph, x.to(DEV).requires_grad_(True), *(t.clone() for t in args), **extra)
    assert not launches, launches


# ---------------------------------------------------------------- I3: no stale entry for a source without a version counter
def test_i3_eids_renumbered_in_place_inside_inference_mode_are_seen(monkeypatch):
    """Inside torch.inference_mode(): build a graph, run the layer, renumber the eids IN PLACE (the permutation and the
    inverse_indices handling of tests.util.permute_eids, written with copy_ into the existing tensors), then run the kind-0 fused-GAT
    pair of tests/test_gpu_ops.py::test_fused_gat_separate_coo on the graph's own tensors: the results are the oracle's for the
    renumbered ids.  (An inference tensor has no version counter; the rule of DESIGN.md: a lookup with such a source never hits.)"""
    from het_amd.kernels import K
    from het_amd.layers import HET_RGATLayer
    from oracle import ops as O
    from tests.util import to64
    H, D, slope = 4, 16, 0.2
    with torch.inference_mode():
        g = random_graph(seed=21, n=300, r=4, e=5000)
        g.to_(DEV)
        N, E = g.get_num_nodes(), g.get_num_edges()
        gen = torch.Generator().manual_seed(9)
        feat, el, er, go = (torch.randn(E, H, D, generator=gen), torch.randn(E, H, generator=gen), torch.randn(E, H, generator=gen),
                            torch.randn(N, H, D, generator=gen))

        def op_pair():
            s = g.get_separate_coo_original()
            idx = (s["eids"], s["rel_ptrs"], s["row_indices"], s["col_indices"])
            sm, ex, ret = (torch.full((N, H), 7.0, device=DEV), torch.full((E, H), 7.0, device=DEV), torch.full((N, H, D), 7.0, device=DEV))
            f, l, r_ = feat.to(DEV), el.to(DEV), er.to(DEV)
            K.relational_fused_gat_separate_coo(*idx, 0, {}, f, l, r_, sm, ex, ret, slope)
            gf, gl, gr = (torch.full_like(t, float("nan")) for t in (f, l, r_))
            K.backward_relational_fused_gat_separate_coo(*idx, 0, {}, f, l, r_, sm, ex, ret, go.to(DEV), gf, gl, gr, slope)
            torch.cuda.synchronize()
            cidx = tuple(t.cpu() for t in idx)
            sm_r, ex_r, ret_r = (torch.empty(N, H, dtype=torch.float64), torch.empty(E, H, dtype=torch.float64),
                                 torch.empty(N, H, D, dtype=torch.float64))
            O.relational_fused_gat_separate_coo(*cidx, 0, {}, to64(feat), to64(el), to64(er), sm_r, ex_r, ret_r, slope)
            gf_r, gl_r, gr_r = torch.zeros_like(to64(feat)), torch.zeros_like(to64(el)), torch.zeros_like(to64(er))
            O.backward_relational_fused_gat_separate_coo(*cidx, 0, {}, to64(feat), to64(el), to64(er), sm_r, ex_r, ret_r, to64(go), gf_r, gl_r,
                                                         gr_r, slope)
            for what, a, r in (("exp", ex, ex_r), ("sum", sm, sm_r), ("ret", ret, ret_r), ("grad_feat", gf, gf_r), ("grad_el", gl, gl_r),
                               ("grad_er", gr, gr_r)):
                assert_close(a, r, what="I3 " + what)
            return sm.clone()

        # 1. the layer (every per-graph tensor it derives is built now) and the op pair on the ids as they are
        torch.manual_seed(3)
        layer = HET_RGATLayer(64, 64, g.get_num_rels(), 4, self_loop=True, dropout=0.0).to(DEV)
        x = torch.randn(N, 64, device=DEV)
        out_before = layer(g, x).clone()
        before = op_pair()
        # 2. renumber in place
        pi = torch.randperm(E, generator=torch.Generator().manual_seed(77)).to(DEV)

        def walk(d):
            for key, v in d.items():
                if isinstance(v, dict):
                    walk(v)
                elif key == "eids":
                    v.copy_(pi[v])
                elif key in ("inverse_indices_row", "inverse_indices_col") and v.numel() == E:
                    moved = torch.empty_like(v)
                    moved[pi] = v
                    v.copy_(moved)
        ptr = g.get_separate_coo_original()["eids"].data_ptr()
        walk(g.graph_data)
        assert g.get_separate_coo_original()["eids"].data_ptr() == ptr and g.get_separate_coo_original()["eids"].is_inference()
        # 3. the same call again: held to the oracle for the renumbered ids
        after = op_pair()
        assert not torch.equal(before, after)  # (el / er rows now belong to other edges: the sums per destination moved)
        # (the layer does not depend on how the edges are numbered: its derived rows must follow the renumbering too)
        assert_close(layer(g, x), out_before.cpu().double(), what="I3 layer output after the renumbering")
