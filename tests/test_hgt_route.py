"""The route of a call of HET_HGTLayerHetero (het_amd/backend/hgt_route.py: decide) on facts alone: no tensor on a device, no
graph.  (a) named calls with the record each must get; (b) over an exhaustive small grid, the implications the autograd node and
hgt_layer_fused rely on -- what a guard inside HgtAttentionFunction.forward and predicates re-derived in its backward used to assert
-- and the short forms of NATIVE and of the node-major conditions against their long forms; (c) the three facts that read the graph
are asked for only where they decide.  tests/test_gpu_hgt_route.py is the check that these records are what runs."""
import itertools

import pytest

from het_amd import kernels as _k
from het_amd.backend import hgt_fused_layer as FL
from het_amd.backend import hgt_route as RT

N = 1000
SUM_SHAPES = [(S, KS, XO) for S in (0, 1, 3, 5, 7, 8, 9, 10) for KS in (32, 64, 128) for XO in (16, 32, 64)]


def _node_sum_ok(S, KS, XO):
    """kernels.node_rows_matmul_sum_ok as an MI355X answers it (csrc/node_sum.hip: het_node_rows_matmul_sum_ok): the library compares
    the kernel's LDS need at 4 waves with the budget of the device it finds, so without a device it refuses most shapes.  160 KiB of
    LDS per workgroup; test_node_sum_stand_in_is_the_library_on_the_gpu holds the two together."""
    if not (1 <= S <= 9 and KS in (32, 64) and XO in (32, 64)):
        return False
    return 4 * (S * KS * XO + 4 * (32 * (max(KS, XO) + 4) + (S + 1) * 32)) <= 160 * 1024


@pytest.fixture(autouse=True)
def _mi355x_shapes(request, monkeypatch):
    if "gpu" not in request.keywords:
        monkeypatch.setattr(_k, "node_rows_matmul_sum_ok", _node_sum_ok)


@pytest.mark.gpu
def test_node_sum_stand_in_is_the_library_on_the_gpu():
    assert [_k.node_rows_matmul_sum_ok(*s) for s in SUM_SHAPES] == [_node_sum_ok(*s) for s in SUM_SHAPES]


def _facts(H=8, K=64, out=64, **kw):
    """The facts of a layer of H heads, K -> out, as layers.py builds them (the bench default: a full graph on the GPU)."""
    d_pad = FL._padded_head(out // H)
    f = dict(cuda=True, bf16=False, dim=2, N=N, K_padded=next((w for w in (32, 64, 128) if w >= K), K), H=H, d_pad=d_pad,
             groups=FL._head_groups(H, d_pad), out_dim=out, plan=True, fused=True, edges=True, lists=True, lists_present=True)
    f.update(kw)
    return RT.Facts(**f)


def _route(H=8, K=64, out=64, S_dst=0.42, rels=(1, 2, 1), canonical=True, asked=None, **kw):
    """decide's record.  ``S_dst``: the destinations with in-edges as a fraction of N; ``rels``: the relations leaving each node
    type; ``asked``: a list that receives the name of every lazily supplied fact that was evaluated."""
    asked = [] if asked is None else asked
    lazy = lambda name, value: lambda: (asked.append(name), value)[1]
    return RT.decide(_facts(H, K, out, **kw), lazy("canonical", canonical), lazy("num_dst_rows", int(S_dst * N)), lazy("rels_per_type", list(rels)))


def _is(r, path, **fields):
    assert r.path == path, r
    for name, want in fields.items():
        assert getattr(r, name) == want, (name, r)


def test_named_calls():
    # the bench default: 8 heads, 64 -> 64, fp32, 42 % of the nodes have in-edges
    _is(_route(), "fused", Kp=64, d_pad=8, groups=1, Xg=64, native_bf16=False, compact_dst=True, out_proj="rows_scatter", split_kv=True,
        split_q=True, dx="node_major")
    _is(_route(S_dst=0.9), "fused", compact_dst=False, out_proj="typed_gemm", dx="node_major")
    _is(_route(S_dst=0.9, compact_dst_below=2.0), "fused", compact_dst=True, out_proj="rows_scatter")
    _is(_route(compact_dst_below=0.0), "fused", compact_dst=False, out_proj="typed_gemm")
    _is(_route(S_dst=0.8), "fused", compact_dst=False)  # (S_dst < 0.8 N, strictly)
    # rows wider than the row kernels take: the heads in two passes of 128 floats; 2 * Xg = 256 is outside the split dX / dW
    _is(_route(8, 64, 256), "fused", groups=2, Xg=128, out_proj="gemm_index_copy", split_kv=False, split_q=True, dx="per_relation")
    _is(_route(2, 32, 256), "fused", d_pad=128, groups=2, Xg=128, split_kv=False, dx="per_relation")
    _is(_route(4, 128, 128), "fused", Kp=128, groups=1, Xg=128, out_proj="rows_scatter", split_kv=False, split_q=True, dx="per_relation")
    _is(_route(4, 128, 64), "fused", Kp=128, Xg=64, split_kv=True, split_q=True, dx="per_relation")  # an input width of 128
    _is(_route(8, 64, 32), "fused", Xg=64, out_proj="rows_scatter", dx="node_major")  # heads of 4 floats padded to 8
    _is(_route(2, 64, 10), "fused", d_pad=8, groups=1, Xg=16, out_proj="gemm_index_copy", split_kv=True, split_q=False, dx="per_relation")
    _is(_route(2, 64, 10, S_dst=0.9), "fused", out_proj="typed_gemm")
    _is(_route(4, 100, 64), "fused", Kp=128, dx="per_relation")  # an input width of 100 pads to 128
    _is(_route(2, 16, 32), "fused", Kp=32, Xg=32, dx="node_major")
    _is(_route(1, 64, 256), "composition")  # one head wider than 128 floats: no split fits
    assert FL._head_groups(1, 256) is None and FL._head_groups(3, 16) is None
    _is(_route(3, 64, 48), "composition")  # rows of 48 floats
    # 1 + 2 * 3 = 7 sources fit the LDS of the node-major pass, 1 + 2 * 4 = 9 do not
    assert _k.node_rows_matmul_sum_ok(7, 64, 64) and not _k.node_rows_matmul_sum_ok(9, 64, 64)
    _is(_route(4, 64, 64, rels=(1, 3, 0)), "fused", dx="node_major")
    _is(_route(4, 64, 64, rels=(1, 4, 0)), "fused", split_kv=True, dx="per_relation")
    _is(_route(4, 64, 64, rels=(1, 4, 0), bf16=True), "fused", native_bf16=True, out_proj="bf16_rows", dx="fp32_buffer")
    _is(_route(4, 64, 64, typed_runs=True), "fused", dx="per_relation")  # a sampled block
    # bf16
    _is(_route(4, 64, 64, bf16=True), "fused", native_bf16=True, groups=1, compact_dst=True, out_proj="bf16_rows", split_kv=True,
        split_q=True, dx="node_major")
    _is(_route(4, 64, 64, bf16=True, S_dst=0.9), "fused", native_bf16=True, compact_dst=False, out_proj="bf16_rows")
    _is(_route(bf16=True), "fused", native_bf16=True)
    _is(_route(2, 32, 32, bf16=True), "fused", native_bf16=True, Xg=32)
    _is(_route(4, 64, 8, bf16=True), "upcast")   # the output projection: 8 columns
    _is(_route(4, 128, 128, bf16=True), "upcast")
    _is(_route(4, 128, 64, bf16=True), "upcast")  # an input width of 128
    _is(_route(4, 100, 64, bf16=True), "upcast")
    _is(_route(8, 64, 256, bf16=True), "upcast")
    _is(_route(4, 64, 64, bf16=True, typed_runs=True), "upcast")
    _is(_route(4, 64, 16, bf16=True), "upcast")  # rows of 32, input 64: the output projection of 16 columns alone (use_norm or not)
    _is(_route(4, 64, 64, bf16=True, fused=False), "upcast")
    _is(_route(4, 64, 64, bf16=True, canonical=False), "upcast")
    _is(_route(4, 64, 64, bf16=True, cuda=False), "upcast")
    # no fused path
    _is(_route(canonical=False), "composition", score="compact", direct=True)
    _is(_route(canonical=False, weights_first_flag=True), "weights_first", score="per_edge")  # (never on the lists' rows)
    _is(_route(canonical=False, weights_first_flag=True, compact_flag=True), "weights_first", score="per_edge")
    _is(_route(canonical=False, weights_first_flag=True, fused_attn_score_flag=True), "weights_first", score="fused_score")
    _is(_route(weights_first_flag=True), "fused")  # (the flag is looked at off the fused path only)
    for off in (dict(fused=False), dict(plan=False), dict(cuda=False), dict(dim=3), dict(edges=False),
                dict(lists=False, lists_present=False)):
        _is(_route(**off), "composition")
        _is(_route(**off, weights_first_flag=True), "weights_first")
        _is(_route(**off, bf16=True), "upcast")
    # the score of the composition
    _is(_route(fused=False, fused_attn_score_flag=True, compact_flag=True), "composition", score="fused_score")
    _is(_route(fused=False, compact_flag=True), "composition", score="compact", direct=False)
    _is(_route(fused=False, compact_flag=True, direct_flag=True), "composition", score="compact", direct=True)
    _is(_route(fused=False), "composition", score="compact", direct=True)  # the lists are there: formed on their rows
    _is(_route(fused=False, lists_present=False), "composition", score="per_edge", direct=True)
    _is(_route(fused=False, cuda=False), "composition", score="per_edge")
    _is(_route(fused=False, plan=False), "composition", score="per_edge")
    _is(_route(fused=False, plan=False, compact_flag=True), "composition", score="compact", direct=False)


SHAPES = [(8, 64, 64), (4, 64, 64), (1, 32, 32), (2, 32, 64), (4, 64, 8), (4, 64, 16), (2, 64, 10), (4, 100, 64), (2, 16, 32), (4, 128, 128),
          (4, 128, 64), (8, 64, 256), (2, 32, 256), (8, 256, 64), (1, 64, 256), (3, 64, 48), (16, 64, 128), (8, 32, 128)]
BOOLS = (False, True)


def test_properties_over_the_grid():
    seen, points = set(), 0
    for (H, K, out), bf16, fused, cuda, canonical, typed_runs, weights_first, S_dst, rels, below in itertools.product(
            SHAPES, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, (0.42, 0.9), ((1, 2, 1), (1, 3, 0), (1, 4, 0)), (0.0, 0.8)):
        kw = dict(H=H, K=K, out=out, bf16=bf16, fused=fused, cuda=cuda, canonical=canonical, typed_runs=typed_runs,
                  weights_first_flag=weights_first, S_dst=S_dst, rels=rels, compact_dst_below=below)
        r = _route(**kw)
        points += 1
        seen.add((r.path, r.out_proj, r.dx))
        assert r.path in ("upcast", "fused", "weights_first", "composition"), (kw, r)
        assert not (r.path == "upcast" and not bf16), (kw, r)
        if r.path != "fused":
            assert r[1:11] == (None,) * 4 + (False, False, None, False, False, None), (kw, r)
            assert (r.path == "upcast") == bf16 and (bf16 or (r.path == "weights_first") == weights_first), (kw, r)
            assert (r.score is not None) == (r.path != "upcast") and (r.path, r.score) != ("weights_first", "compact"), (kw, r)
            continue
        f = _facts(H, K, out)
        assert fused and cuda and canonical and r.native_bf16 == bf16, (kw, r)
        assert (r.Kp, r.d_pad, r.groups, r.Xg) == (f.K_padded, f.d_pad, f.groups, H * f.d_pad // f.groups), (kw, r)
        assert _k.hgt_compact_shape_ok(H // r.groups, r.d_pad), (kw, r)
        assert r.compact_dst == (S_dst < below), (kw, r)
        assert r.split_kv == _k.rows_matmul_backward_split_ok(1, r.Kp, 2 * r.Xg) and r.split_q == _k.rows_matmul_backward_split_ok(1, r.Kp, r.Xg)
        # what HgtAttentionFunction and hgt_layer_fused rely on
        if r.native_bf16:
            assert r.groups == 1 and r.split_kv and r.split_q and not typed_runs and r.out_proj == "bf16_rows", (kw, r)
            assert _k.rows_matmul_bf16_ok(r.Kp, 2 * r.Xg) and _k.rows_matmul_bf16_ok(r.Kp, r.Xg) and _k.rows_matmul_bf16_ok(out, out), (kw, r)
        if r.dx == "node_major":
            assert r.split_kv and not typed_runs and all(_k.node_rows_matmul_sum_ok(1 + 2 * n, r.Xg, r.Kp) for n in rels), (kw, r)
        assert (r.dx == "fp32_buffer") <= r.native_bf16 and (r.dx == "per_relation") <= (not bf16), (kw, r)
        assert (r.out_proj == "rows_scatter") <= r.compact_dst and (r.out_proj == "typed_gemm") <= (not r.compact_dst), (kw, r)
        assert (r.out_proj == "rows_scatter") <= _k.rows_matmul_backward_split_ok(1, out, out), (kw, r)
        assert r.score is None, (kw, r)
    assert points == 18 * 2 ** 6 * 2 * 3 * 2
    assert {s[0] for s in seen} == {"upcast", "fused", "weights_first", "composition"}
    assert {s[1] for s in seen} == {None, "bf16_rows", "typed_gemm", "rows_scatter", "gemm_index_copy"}
    assert {s[2] for s in seen} == {None, "node_major", "fp32_buffer", "per_relation"}


def test_short_forms_equal_the_long_forms():
    """decide's NATIVE and node-major conditions leave out what their other conditions imply at every width the layer can produce
    (d_pad a power of two >= 8, the padded input width): one head group, rows_matmul_bf16_ok(Kp, 2X), both
    rows_matmul_backward_split_ok of the attention node (NATIVE), and split_kv (node-major).  The long forms, as the layer and the
    autograd node spelled them before, over 7 head counts x 12 head widths x 8 input widths x 2 x 2 = 2688 points."""
    points = 0
    for H, d_k, K, typed_runs, rels in itertools.product((1, 2, 3, 4, 8, 16, 32), (1, 2, 4, 5, 8, 12, 16, 32, 33, 64, 128, 256),
                                                         (8, 16, 32, 48, 64, 100, 128, 256), BOOLS, ((1, 3, 0), (1, 4, 0))):
        f = _facts(H, K, H * d_k, typed_runs=typed_runs)
        Kp, X, out = f.K_padded, H * f.d_pad, H * d_k
        points += 1
        native = (not typed_runs and X in (32, 64) and Kp in (32, 64) and f.groups == 1 and _k.rows_matmul_bf16_ok(Kp, 2 * X)
                  and _k.rows_matmul_bf16_ok(out, out) and _k.rows_matmul_backward_split_ok(1, Kp, 2 * X)
                  and _k.rows_matmul_backward_split_ok(1, Kp, X))
        r = _route(H, K, out, typed_runs=typed_runs, rels=rels, bf16=True)
        assert (r.path, r.native_bf16) == (("fused", True) if native else ("upcast", False)), (H, d_k, K, typed_runs, r)
        r = _route(H, K, out, typed_runs=typed_runs, rels=rels)
        if r.path == "fused":
            node_major = (r.split_kv and not typed_runs and r.Xg in (32, 64) and Kp in (32, 64)
                          and all(_k.node_rows_matmul_sum_ok(1 + 2 * n, r.Xg, Kp) for n in rels))
            assert (r.dx == "node_major") == node_major, (H, d_k, K, typed_runs, rels, r)
        else:
            assert f.groups is None, (H, d_k, K, r)
    assert points == 2688


def test_lazy_facts_are_asked_only_where_they_decide():
    """canonical reads every edge of a graph the first time, num_dst_rows builds the destination lists, rels_per_type reads the
    relations' node types back to the host: none is asked off the fused path, canonical after every cheap condition of FUSED_OK and
    not for a bf16 input outside NATIVE, rels_per_type only where the cheap conditions of the node-major pass hold."""
    def asked(*shape, **kw):
        names = []
        _route(*shape, asked=names, **kw)
        return names
    assert asked() == ["canonical", "num_dst_rows", "rels_per_type"]
    assert asked(bf16=True) == ["canonical", "num_dst_rows", "rels_per_type"]
    assert asked(canonical=False) == ["canonical"]
    assert asked(canonical=False, bf16=True) == ["canonical"]
    for shape in ((4, 128, 128), (4, 128, 64), (8, 64, 256), (2, 64, 10), (4, 100, 64)):  # Xg or Kp outside 32 / 64
        assert asked(*shape) == ["canonical", "num_dst_rows"], shape
        assert asked(*shape, bf16=True) == [], shape
    assert asked(typed_runs=True) == ["canonical", "num_dst_rows"]
    assert asked(typed_runs=True, bf16=True) == []
    assert asked(4, 64, 16, bf16=True) == []
    for off in (dict(fused=False), dict(plan=False), dict(cuda=False), dict(dim=3), dict(edges=False), dict(lists=False),
                dict(groups=None)):
        for more in (dict(), dict(bf16=True), dict(weights_first_flag=True)):
            assert asked(**off, **more) == [], (off, more)
