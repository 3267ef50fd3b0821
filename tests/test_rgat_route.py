"""The route of a call of HET_RGATLayer (het_amd/backend/rgat_route.py: decide, with_backward) on facts alone: no tensor on a
device, no graph.  (a) named calls with the record each must get; (b) over an exhaustive small grid, the implications the autograd
nodes rely on -- what asserts inside a backward on the GPU used to guard; (c) the two facts that may read the graph's lists are
asked for only where they decide.  The GPU files that count calls per path (test_gpu_rgat_backward_routes.py, _step_lean,
_forward_only, _bf16, _bf16_train, _attention, test_gpu_dist.py) are the check that these records are what runs."""
import itertools

import pytest

from het_amd import kernels as _k
from het_amd.backend import rgat_route as RT

N = 1000
GEMM_SHAPES = [(R, H, K, D) for R in (1, 4, 8, 9) for H, K, D in ((4, 64, 16), (4, 64, 32), (8, 128, 4), (8, 128, 1), (2, 32, 16), (3, 64, 16),
                                                                  (2, 64, 16), (4, 32, 8), (4, 64, 8), (16, 32, 4), (4, 128, 16), (4, 256, 16))]


def _node_gemm_ok(R, H, K, D):
    """kernels.rgat_node_gemm_ok as an MI355X answers it (csrc/node_gemm.hip: het_rgat_node_gemm_ok): the library compares the
    kernel's LDS need with the budget of the device it finds, so without a device it refuses every shape.  160 KiB of LDS per
    workgroup; test_node_gemm_stand_in_is_the_library_on_the_gpu holds the two together."""
    if not (1 <= R <= 8 and H in (1, 2, 4, 8) and R * H <= 32 and D > 0 and K in (32, 64) and H * D in (32, 64)):
        return False
    KS, rhp = H * D, (R * H + 7) // 8 * 8
    return 4 * ((1 + R) * KS * K + rhp * K + 4 * (32 * (max(KS, K) + 4) + (2 + R) * 32)) <= 160 * 1024


@pytest.fixture(autouse=True)
def _mi355x_shapes(request, monkeypatch):
    if "gpu" not in request.keywords:
        monkeypatch.setattr(_k, "rgat_node_gemm_ok", _node_gemm_ok)


@pytest.mark.gpu
def test_node_gemm_stand_in_is_the_library_on_the_gpu():
    assert [_k.rgat_node_gemm_ok(*s) for s in GEMM_SHAPES] == [_node_gemm_ok(*s) for s in GEMM_SHAPES]


def _facts(**kw):
    f = dict(cuda=True, bf16=False, dim=2, N=N, K=64, H=4, D=16, R=4, edges=True, slope=0.2, grad=True, halo=False, num_dst=None,
             plan=True, lists=True)
    f.update(kw)
    f.setdefault("K_padded", next((w for w in (32, 64, 128) if w >= f["K"]), f["K"]))
    return RT.Facts(**f)


def _route(below=True, asked=None, **kw):
    """decide's record, the fp32 node's with the backward it resolves when the backward runs.  ``below``: every edge ends below nd;
    ``asked``: a list that receives the name of every lazily supplied fact that was evaluated."""
    asked = [] if asked is None else asked

    def dst_below(nd):
        assert nd == (N if kw.get("num_dst") is None else min(kw["num_dst"], N))
        asked.append("dst_below")
        return below

    def attn_dot_only(R, H, K, D):
        asked.append("attn_dot_only")
        return True
    r = RT.decide(_facts(**kw), dst_below, attn_dot_only)
    return RT.with_backward(r, lambda: below) if r.path == "node" else r


def _is(r, path, **fields):
    assert r.path == path, r
    for name, want in fields.items():
        assert getattr(r, name) == want, (name, r)


HALO = dict(halo=True, self_loop=True, num_dst=N)
BF16_TRAIN = dict(bf16=True, bf16_training=True)


def test_named_calls():
    _is(_route(), "node", Kp=64, Dp=16, compact=True, direct=True, mulfirst=True, run_sums=True, halo=False, backward="node_major",
        attn_in_pass=True)
    _is(_route(grad=False), "eval", compact=True, mulfirst=True, run_sums=True)
    _is(_route(grad=False, forward_only=False), "node", backward="node_major")
    _is(_route(D=32), "node", backward="generic", attn_in_pass=False)  # rows of 128
    _is(_route(num_dst=N // 2, below=False), "node", backward="generic", attn_in_pass=False)
    _is(_route(num_dst=N // 2, below=True), "node", backward="node_major", attn_in_pass=True)  # a block
    _is(_route(literal_er=True), "node", compact=True, mulfirst=False, backward="generic", attn_in_pass=False)
    _is(_route(literal_er=True, mulfirst_flag=True), "node", mulfirst=True, backward="node_major")  # the layer flag asks for it
    _is(_route(per_edge=True), "node", compact=False, direct=False, run_sums=False, backward=None, attn_in_pass=False)
    _is(_route(per_edge=True, compact_flag=True, direct_flag=False), "node", compact=True, direct=False, backward="node_major")
    _is(_route(lists=False), "node", compact=False, backward=None)
    _is(_route(D=8), "node", Kp=64, Dp=8, run_sums=False, backward="node_major", attn_in_pass=False)  # heads below 16: no run sums
    _is(_route(K=256, grad=False), "eval", Kp=256, Dp=16)  # the any-shape projection
    _is(_route(K=256, grad=False, bf16=True), "upcast")  # rgat_bf16_shape_ok: an input width of 32 / 64 / 128
    _is(_route(K=256, literal_er=True), "composition")  # ... which needs the distinct rows AND the folded weight
    _is(_route(K=256, per_edge=True), "composition")
    _is(_route(H=16, K=32, D=4), "node", compact=True, mulfirst=False, backward="generic")  # 16 heads: outside the one-head row-dot
    assert not _k.rgat_node_gemm_ok(9, 4, 64, 16)  # (read, not assumed: the node-major pass takes at most 8 relations)
    _is(_route(R=9), "node", attn_in_pass=False, backward="generic")
    _is(_route(bf16=True, grad=False), "eval_bf16", compact=True, mulfirst=True, run_sums=True)
    _is(_route(bf16=True, grad=False, literal_er=True), "eval_bf16", mulfirst=True)  # no literal er in bf16
    _is(_route(bf16=True), "upcast")
    _is(_route(**BF16_TRAIN), "train_bf16", compact=True, mulfirst=True, run_sums=True, halo=False, backward="node_major", attn_in_pass=True)
    _is(_route(**BF16_TRAIN, grad=False), "eval_bf16")
    _is(_route(**BF16_TRAIN, R=9), "upcast")
    _is(_route(**BF16_TRAIN, D=32), "upcast")
    _is(_route(**BF16_TRAIN, K=128), "upcast")  # the node-major pass: an input width of 32 or 64
    _is(_route(**BF16_TRAIN, num_dst=N // 2, below=False), "upcast")
    _is(_route(**BF16_TRAIN, num_dst=N // 2, below=True), "train_bf16")
    _is(_route(**BF16_TRAIN, per_edge=True), "upcast")
    _is(_route(**BF16_TRAIN, N=2 ** 29), "upcast")
    _is(_route(bf16=True, grad=False, forward_only=False), "upcast")
    _is(_route(bf16=True, grad=False, N=2 ** 29), "upcast")  # N * R = 2^31
    # N * R = 2^31: the groupings fall back to the per-edge form, so no run sums, no evaluation form, no attention gradient in the pass
    _is(_route(grad=False, N=2 ** 29), "node", run_sums=False, backward="node_major", attn_in_pass=False)
    _is(_route(N=2 ** 29), "node", compact=True, run_sums=False, backward="node_major", attn_in_pass=False)
    _is(_route(N=2 ** 29 - 1), "node", run_sums=True, attn_in_pass=True)
    _is(_route(**dict(HALO, N=2 ** 29)), "node", halo=True, run_sums=False, backward="node_major", attn_in_pass=False)
    _is(_route(**dict(HALO, N=2 ** 29), D=32), "node", halo=True, run_sums=False, backward="per_relation", attn_in_pass=False)
    # the reference CLI's 8 classes over 8 heads: every head zero-padded to 4 floats
    _is(_route(H=8, K=128, D=1), "node", Kp=128, Dp=4, compact=True, mulfirst=True, run_sums=False, attn_in_pass=False)
    _is(_route(H=8, K=128, D=1, pad_heads=False), "composition", Kp=128, Dp=1)
    _is(_route(K=100), "node", Kp=128, Dp=16)  # an input width of 100 pads to 128
    _is(_route(cuda=False), "composition")
    _is(_route(cuda=False, bf16=True), "upcast")
    _is(_route(reference_op_sequence=True), "reference")
    _is(_route(reference_op_sequence=True, bf16=True), "upcast")
    _is(_route(op_by_op=True), "composition")
    _is(_route(op_by_op=True, bf16=True, grad=False), "upcast")
    _is(_route(gat_edge_parallel=False), "composition")
    _is(_route(plan=False), "composition")
    _is(_route(edges=False), "composition")
    _is(_route(dim=3), "composition")
    _is(_route(slope=-0.1), "composition")
    _is(_route(H=3), "composition")  # rows of 48 floats
    _is(_route(H=16, K=32, D=4, mulfirst_flag=True), "composition")  # the layer asks for a folded weight outside the row-dot's shapes
    _is(_route(**HALO), "node", halo=True, compact=True, mulfirst=True, backward="node_major", attn_in_pass=True)
    _is(_route(**HALO, grad=False), "node", halo=True)  # no evaluation form with a halo
    _is(_route(**HALO, op_by_op=True), "node", halo=True)  # (not looked at with a halo)
    _is(_route(**dict(HALO, self_loop=False)), "composition")  # not served: forward_with_halo returns None
    _is(_route(**HALO, reference_op_sequence=True), "composition")
    _is(_route(**HALO, per_edge=True), "composition")
    _is(_route(**HALO, literal_er=True), "composition")
    _is(_route(**HALO, K=256), "composition")  # rows_linear_bias_ok / rows_matmul_backward_split_ok
    _is(_route(**HALO, H=8, K=128, D=1), "composition")  # heads are not padded with a halo
    _is(_route(**HALO, D=32), "node", halo=True, backward="per_relation", attn_in_pass=True)
    _is(_route(**HALO, bf16=True), "upcast")  # ... then the halo decision on the fp32 copy: the rows above
    _is(_route(**HALO, **BF16_TRAIN), "upcast")


SHAPES = [(4, 64, 16), (4, 64, 32), (8, 128, 1), (2, 32, 16), (3, 64, 16)]
BOOLS = (False, True)


def test_properties_over_the_grid():
    seen = set()
    for (bf16, grad, training, halo, self_loop, per_edge, literal_er, forward_only, pad_heads, R, (H, K, D), prefix, cuda) in itertools.product(
            BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, (4, 9), SHAPES, BOOLS, BOOLS):
        kw = dict(bf16=bf16, grad=grad, bf16_training=training, halo=halo, self_loop=self_loop, per_edge=per_edge, literal_er=literal_er,
                  forward_only=forward_only, pad_heads=pad_heads, R=R, H=H, K=K, D=D, cuda=cuda, num_dst=N // 2 if prefix or halo else None)
        r = _route(below=prefix or halo, **kw)  # (a partition's edges point at owned nodes)
        seen.add(r.path)
        assert r.path in ("upcast", "composition", "node", "eval", "eval_bf16", "train_bf16"), r
        assert (r.R, r.H) == (R, H) and r.halo == (halo and r.path == "node"), (kw, r)
        if r.path in ("upcast", "composition"):
            assert r[5:] == (False,) * 5 + (None, False) and (r.Kp, r.Dp) == (K, D), (kw, r)
            assert (r.path == "upcast") == bf16, (kw, r)
            continue
        assert cuda and bf16 == (r.path in ("eval_bf16", "train_bf16")), (kw, r)
        if r.path == "train_bf16":
            assert (r.backward, r.attn_in_pass, r.halo) == ("node_major", True, False) and grad and training, (kw, r)
            assert K in (32, 64) and H * r.Dp in (32, 64), (kw, r)
        if r.path in ("eval", "eval_bf16"):
            assert not grad and not r.halo and forward_only and r.run_sums and r.backward is None and not r.attn_in_pass, (kw, r)
        if bf16:
            assert r.compact and r.mulfirst and r.run_sums and r.Kp in (32, 64, 128), (kw, r)
        if r.halo:
            assert r.compact and r.mulfirst and self_loop and (r.Kp, r.Dp) == (K, D) and r.backward in ("node_major", "per_relation"), (kw, r)
        if r.attn_in_pass:
            assert r.run_sums and R <= 8 and r.backward in ("node_major", "per_relation"), (kw, r)
        if r.backward == "node_major":
            assert r.mulfirst and _k.rgat_node_gemm_ok(R, H, r.Kp, r.Dp) and (prefix or halo), (kw, r)
        if r.backward == "per_relation":
            assert r.halo, (kw, r)
        assert (r.backward is not None) == (r.compact and r.path in ("node", "train_bf16")), (kw, r)
        assert r.run_sums == (r.compact and _k.rgat_runs_shape_ok(H, r.Dp) and N * R < 2 ** 31), (kw, r)
        assert not (r.compact and per_edge) and (r.mulfirst or literal_er) and (pad_heads or (r.Kp, r.Dp) == (K, D)), (kw, r)
    assert seen == {"upcast", "composition", "node", "eval", "eval_bf16", "train_bf16"}


def test_lazy_facts_are_asked_only_where_they_decide():
    """dst_below costs a device reduction the first time: decide asks it for the bf16 training decision alone, after every other
    condition (the fp32 node resolves its backward when the backward runs); attn_dot_only only where the call would run on the
    per-edge dataflow with the literal er."""
    def asked(**kw):
        names = []
        _route(asked=names, **kw)
        return names
    for kw in (dict(), dict(grad=False), dict(D=32), dict(num_dst=N // 2), dict(bf16=True), dict(bf16=True, grad=False), HALO,
               dict(per_edge=True), dict(literal_er=True), dict(cuda=False), dict(**BF16_TRAIN, R=9), dict(**BF16_TRAIN, D=32),
               dict(**BF16_TRAIN, K=128), dict(**BF16_TRAIN, per_edge=True), dict(**BF16_TRAIN, grad=False)):
        assert asked(**kw) == [], kw
    assert asked(**BF16_TRAIN) == ["dst_below"]
    assert asked(per_edge=True, literal_er=True) == ["attn_dot_only"]
    assert asked(per_edge=True, literal_er=True, plan=False) == []
    names = []
    r = RT.decide(_facts(per_edge=True, literal_er=True), lambda nd: True, lambda R, H, K, D: bool(names.append((K, D))))
    assert names == [(64, 16)] and r.path == "composition"  # (nothing to pad: the one pair of widths is tried once)
    # (asked at the padded widths; the layer's own, 100 wide, are outside the matrix-core projection whatever the lists say)
    names = []
    r = RT.decide(_facts(per_edge=True, literal_er=True, K=100), lambda nd: True, lambda R, H, K, D: bool(names.append((K, D))))
    assert names == [(128, 16)] and r.path == "composition"
