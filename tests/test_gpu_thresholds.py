"""GPU parity at the counts where the grouped kernels change code path (tests/util.py::ladder_graph): segment lengths of exactly
HET_PACK_T = 32, the RGAT backward's pack threshold 64, HET_ITEM_MAX = 256 and the RGAT hub threshold 256 (and one either side),
destinations whose runs add up to a threshold, rows per relation around the 32 / 64-row tiles and 2048-row chunks of the segment
GEMMs, and relation counts around the R <= 8 switches.  The op cases are the ones of tests/test_gpu_ops.py, run on the ladder graph
against the same fp64 oracle calls, at widths that reach every lanes-per-row instantiation of each op's dispatch."""
import os
import subprocess
import sys

import pytest
import torch

import tests.test_gpu_ops as T
from oracle import ops as O
from tests.test_gpu_ops import K, plan_mode  # noqa: F401  (fixtures)
from tests.util import LADDER, assert_close, assert_ladder, assert_rungs, ladder_counts, ladder_graph, row_ladder_ptrs, to64

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ladder():
    g = ladder_graph(R=5, seed=0)
    assert_ladder(g)
    return g


# ---------------------------------------------------------------- RGAT compact passes
# every (lanes per row, lanes per head) pair of HET_DISPATCH_COOP (coop_shape_ok, coop.hip.h; both GAT files launch through it): rows of
# 32 / 64 / 128 floats, heads of 16 .. 128; D = 16 also runs the forward with el formed from the row (kElMaxRels) and the attention
# gradient in the backward pass
RUN_SHAPES = [(2, 16), (1, 32), (4, 16), (2, 32), (1, 64), (8, 16), (4, 32), (2, 64), (1, 128)]
# shapes outside the cooperative pairs, one per lanes-per-row case 1 .. 64 of HET_DISPATCH_LPR (LPR = H * D / 4; at LPR 8 / 16 / 32
# heads of 8 floats, which the cooperative kernels do not take)
LPR_SHAPES = [(1, 4), (2, 4), (2, 8), (4, 8), (8, 8), (16, 8), (8, 32)]


@pytest.mark.parametrize("H,D", RUN_SHAPES)
def test_rgat_ladder_run_sums(K, ladder, H, D):
    T.rgat_run_sums_case(K, ladder, H, D, fold=True, bias=True)


def test_rgat_ladder_run_sums_without_fold(K, ladder):
    T.rgat_run_sums_case(K, ladder, 4, 16, fold=False, bias=False)


# the non-run form: HET_DISPATCH_LPR 1 .. 64 and every cooperative pair
@pytest.mark.parametrize("H,D", LPR_SHAPES + RUN_SHAPES)
def test_rgat_ladder_compact_passes(K, ladder, H, D):
    T.rgat_compact_case(K, ladder, H, D, fold=True, bias=True)


# ---------------------------------------------------------------- fused GAT, reference-named op
# the grouped kernels: HET_DISPATCH_LPR 1 .. 64 and every pair of HET_DISPATCH_COOP; (3, 5): the edge kernels
GAT_ALL_LPR = LPR_SHAPES + RUN_SHAPES + [(3, 5)]


@pytest.mark.parametrize("kind,H,D", [(kd, h, d) for kd in (0, 4) for h, d in GAT_ALL_LPR]
                         + [(kd, h, d) for kd in (1, 2, 3) for h, d in ((4, 16), (1, 4), (3, 5))])
def test_fused_gat_ladder(K, plan_mode, ladder, kind, H, D):
    T.fused_gat_case(K, ladder, kind, H, D)


@pytest.mark.parametrize("H,D", [(4, 16), (1, 64), (2, 8)])
def test_fused_gat_ladder_folded_attn_l(ladder, H, D):
    T.folded_attn_l_case(ladder, H, D)


@pytest.mark.parametrize("R", [8, 9])
def test_fused_gat_folded_attn_l_relation_count(R):
    """grad_fold_attn_l in registers up to kFoldRelMax = 8 relations, against the per-relation sums of grad_el * feat of the fp64
    oracle; at 9 the op refuses it with its message, and the autograd node takes the separate weight-gradient pass (same values)."""
    import het_amd.kernels as k
    g = ladder_graph(R=R, seed=2)
    assert_rungs(ladder_counts(g)["in_rel"], LADDER, "in-degree per (relation, destination)")
    T.folded_attn_l_case(g, 4, 16)
    sc = g.get_separate_coo_original()
    s = {kk: v.to(DEV) for kk, v in sc.items()}
    E, N, H, D, slope = g.get_num_edges(), g.get_num_nodes(), 4, 16, 0.2
    gen = torch.Generator().manual_seed(3)
    feat, attn = torch.randn(E, H, D, generator=gen), torch.randn(R, H, D, generator=gen)
    el, er, go = torch.randn(E, H, generator=gen), torch.randn(E, H, generator=gen), torch.randn(N, H, D, generator=gen)
    idx = (s["eids"], s["rel_ptrs"], s["row_indices"], s["col_indices"])
    sm, ex, ret, exs = torch.empty(N, H, device=DEV), torch.empty(E, H, device=DEV), torch.empty(N, H, D, device=DEV), torch.empty(E, H, device=DEV)
    f, a, l, r_ = feat.to(DEV), attn.to(DEV), el.to(DEV), er.to(DEV)
    assert k.fused_gat_forward(*idx, 0, {}, f, l, r_, sm, ex, ret, slope, exs)
    gf, gl, ga = torch.full_like(f, float("nan")), torch.full_like(l, float("nan")), torch.zeros_like(a)

    def backward():
        k.fused_gat_backward(*idx, 0, {}, f, l, r_, sm, ex, ret, go.to(DEV), gf, gl, gl, slope, exs, fold_attn_l=a, grad_fold_attn_l=ga)
    if R > 8:
        with pytest.raises(Exception, match="grad_fold_attn_l needs fold_attn_l and at most 8 relations"):
            backward()
        return
    backward()
    idxc = (sc["eids"], sc["rel_ptrs"], sc["row_indices"], sc["col_indices"])
    sm_r, ex_r, ret_r = (torch.empty(N, H, dtype=torch.float64), torch.empty(E, H, dtype=torch.float64),
                         torch.empty(N, H, D, dtype=torch.float64))
    O.relational_fused_gat_separate_coo(*idxc, 0, {}, to64(feat), to64(el), to64(er), sm_r, ex_r, ret_r, slope)
    gf_r, gl_r, gr_r = torch.zeros_like(to64(feat)), torch.zeros_like(to64(el)), torch.zeros_like(to64(er))
    O.backward_relational_fused_gat_separate_coo(*idxc, 0, {}, to64(feat), to64(el), to64(er), sm_r, ex_r, ret_r, to64(go), gf_r, gl_r,
                                                 gr_r, slope)
    rel_of_eid = torch.empty(E, dtype=torch.int64)  # (edge data is indexed by edge id)
    rel_of_eid[sc["eids"]] = torch.repeat_interleave(torch.arange(R), sc["rel_ptrs"][1:] - sc["rel_ptrs"][:-1])
    assert_close(gl, gl_r, what="grad_el")
    assert_close(gf, gf_r + gl_r.unsqueeze(-1) * to64(attn)[rel_of_eid], what="grad_feat (with grad_el x attn_l)")
    ga_r = torch.zeros(R, H, D, dtype=torch.float64).index_add_(0, rel_of_eid, gl_r.unsqueeze(-1) * to64(feat))
    assert_close(ga, ga_r, what="grad_attn_l")


# ---------------------------------------------------------------- HGT
# every (lanes per row, lanes per head) pair of HET_DISPATCH_HGT_ROWS
HGT_ROWS = [(1, 8), (2, 8), (1, 16), (4, 8), (2, 16), (1, 32), (8, 8), (4, 16), (2, 32), (1, 64), (16, 8), (8, 16), (4, 32), (2, 64),
            (1, 128)]


@pytest.mark.parametrize("H,D", HGT_ROWS)
def test_hgt_ladder_compact_passes(K, ladder, H, D):
    import het_amd.kernels as k
    assert k.hgt_compact_shape_ok(H, D)
    T.hgt_compact_case(K, ladder, H, D)


@pytest.mark.parametrize("H", [1, 2, 4, 8, 16, 3])
def test_hgt_ladder_edge_softmax(K, plan_mode, ladder, H):
    T.hgt_softmax_case(K, ladder, H, 4)


@pytest.mark.parametrize("H,dk", [(8, 8), (4, 16), (1, 64), (2, 32), (1, 128), (2, 6)])
def test_hgt_ladder_fused_message(K, plan_mode, ladder, H, dk):
    T.hgt_message_case(K, ladder, H, dk)


@pytest.mark.parametrize("H,dk", [(8, 8), (2, 6)])
def test_hgt_ladder_fused_attention(K, plan_mode, ladder, H, dk):
    T.hgt_attention_case(K, ladder, H, dk)


# ---------------------------------------------------------------- RGCN, segment sums
@pytest.mark.parametrize("Kd,D", [(16, 16), (64, 64), (7, 3)])
def test_rgcn_ladder_layer1(K, plan_mode, ladder, Kd, D):
    T.rgcn_layer1_case(K, ladder, Kd, D)


@pytest.mark.parametrize("direct", [False, True])
def test_rgcn_ladder_compact_aggregation(K, plan_mode, ladder, direct):
    T.rgcn_compact_case(K, ladder, direct)


@pytest.mark.parametrize("X", [4, 8, 16, 32, 64, 128, 256])
def test_rows_scatter_add_ladder(plan_mode, ladder, X):
    """het_rows_scatter_add_grouped (segments = the ladder's in-degrees: packs, long segments, split ones) and the atomics kernel."""
    import het_amd.kernels as k
    idx = ladder.get_separate_coo_original()["col_indices"]
    N, E = ladder.get_num_nodes(), idx.numel()
    gen = torch.Generator().manual_seed(X)
    src, acc = torch.randn(E, X, generator=gen), torch.randn(N, X, generator=gen)
    got = k.rows_scatter_add_(acc.to(DEV), idx.to(DEV), src.to(DEV))
    assert_close(got, acc.double().index_add_(0, idx, src.double()), what=f"scatter_add X={X}")


# ---------------------------------------------------------------- node-major passes
@pytest.mark.parametrize("H,Kd,D", [(4, 64, 16), (1, 64, 64), (2, 32, 16), (2, 64, 32), (1, 32, 32)])
def test_rgat_node_backward_dx_ladder(ladder, H, Kd, D):
    """het_rgat_node_backward_dx on the ladder's (relation, source) / (relation, destination) lists, against the per-term sum."""
    import het_amd.kernels as k
    R, N = ladder.get_num_rels(), ladder.get_num_nodes()
    assert k.rgat_node_gemm_ok(R, H, Kd, D)
    ss = ladder.get_separate_unique_node_indices_single_sided()
    rp_row, n_row, rp_col, n_col = ss["rel_ptrs_row"], ss["node_indices_row"], ss["rel_ptrs_col"], ss["node_indices_col"]
    gen = torch.Generator().manual_seed(H + Kd)
    X, n_loop = H * D, N - 5
    gh, g_rows = torch.randn(n_loop, X, generator=gen, dtype=torch.float64), torch.randn(n_row.numel(), X, generator=gen, dtype=torch.float64)
    g_er = torch.randn(n_col.numel(), H, generator=gen, dtype=torch.float64)
    loop_w, W = torch.randn(Kd, X, generator=gen, dtype=torch.float64), torch.randn(R, H, Kd, D, generator=gen, dtype=torch.float64)
    wa = torch.randn(R, H, Kd, generator=gen, dtype=torch.float64)
    gx = torch.zeros(N, Kd, dtype=torch.float64)
    gx[:n_loop] += gh @ loop_w.t()
    for r in range(R):
        a, b = int(rp_row[r]), int(rp_row[r + 1])
        gx.index_add_(0, n_row[a:b], g_rows[a:b] @ W[r].permute(1, 0, 2).reshape(Kd, X).t())
        a, b = int(rp_col[r]), int(rp_col[r + 1])
        gx.index_add_(0, n_col[a:b], g_er[a:b] @ wa[r])
    f = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    row_map, dst_map = k.node_row_map(rp_row.to(DEV), n_row.to(DEV), N), k.node_row_map(rp_col.to(DEV), n_col.to(DEV), N)
    out = torch.full((N, Kd), float("nan"), device=DEV)
    k.rgat_node_backward_dx(0, N, n_loop, f(gh), f(loop_w.t()), f(g_rows), f(W.transpose(2, 3)), row_map, f(g_er), f(wa), dst_map, out)
    assert_close(out, gx, what="grad_x")


@pytest.mark.parametrize("R", [1, 7, 8, 9, 12])
def test_node_rows_matmul_sum_relation_count(R):
    """het_node_rows_matmul_sum over one source per relation (+ one identity-mapped source, the self loop), up to kMaxSrc = 9
    sources (rows of 32 floats: 64-float ones run out of LDS before that); more are refused by node_rows_matmul_sum_ok (the layers
    then take their fallback)."""
    import het_amd.kernels as k
    g = ladder_graph(R=R, seed=4, shuffle=False)
    N = g.get_num_nodes()
    ss = g.get_separate_unique_node_indices_single_sided()
    rp, nodes = ss["rel_ptrs_row"], ss["node_indices_row"]
    S = R + 1
    assert k.node_rows_matmul_sum_ok(S, 32, 32) == (S <= 9)
    if S > 9:
        return
    gen = torch.Generator().manual_seed(R)
    rows = torch.randn(nodes.numel(), 32, generator=gen)
    xl = torch.randn(N, 32, generator=gen)
    wts = [torch.randn(32, 32, generator=gen) * 0.2 for _ in range(S)]
    row_map = k.node_row_map(rp.to(DEV), nodes.to(DEV), N)
    want = xl.double() @ wts[R].double()
    m = row_map.cpu().long()
    for r in range(R):
        has = m[r] >= 0
        want[has] += rows.double()[m[r][has]] @ wts[r].double()
    rd = rows.to(DEV)
    sources = [(rd, 0, row_map[r].contiguous(), wts[r].to(DEV)) for r in range(R)] + [(xl.to(DEV), 0, None, wts[R].to(DEV))]
    out = torch.full((N, 32), float("nan"), device=DEV)
    k.node_rows_matmul_sum(0, N, sources, out)
    assert_close(out, want, what=f"node sum of {S} sources")


# ---------------------------------------------------------------- segment GEMMs on the row-count ladder
GEMM_SHAPES = [(3, 7, 5, True), (1, 16, 16, True), (4, 16, 1, False), (4, 64, 16, True), (1, 32, 32, True), (2, 64, 64, True),
               (4, 128, 32, True), (4, 64, 1, True)]


@pytest.mark.parametrize("H,Kd,D,in1head", GEMM_SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_relational_matmul_row_ladder(K, kind, H, Kd, D, in1head):
    """rgnn_relational_matmul fwd / bwd with relations of 0, 1, 31 .. 33, 63 .. 65, 2047 .. 2049 and 4097 rows, boundaries mid-tile."""
    rp = row_ladder_ptrs()
    R, n = rp.numel() - 1, int(rp[-1])
    N = 5000
    gen = torch.Generator().manual_seed(7 + kind)
    W = torch.randn(R, H, Kd, D, generator=gen)
    x = torch.randn(N, Kd, generator=gen) if in1head else torch.randn(N, H, Kd, generator=gen)
    nodes = torch.randint(0, N, (n,), generator=gen)
    if kind == 0:
        d = {"separate_coo_rel_ptrs": rp, "separate_coo_node_indices": nodes, "separate_coo_eids": torch.randperm(n, generator=gen)}
    else:  # distinct nodes inside a relation (a unique (relation, node) list)
        nodes = torch.cat([torch.randperm(N, generator=gen)[: int(rp[r + 1] - rp[r])].sort().values for r in range(R)])
        d = {"unique_srcs_and_dests_rel_ptrs": rp, "unique_srcs_and_dests_node_indices": nodes}
    ref = torch.zeros(n, H, D, dtype=torch.float64)
    O.rgnn_relational_matmul(d, kind, to64(W), to64(x), ref, in1head)
    ret = torch.full((n, H, D), float("nan"), device=DEV)
    K.rgnn_relational_matmul(T._dev(d), kind, W.to(DEV), x.to(DEV), ret, in1head)
    assert_close(ret, ref, what="ret")
    go = torch.randn(n, H, D, generator=gen)
    gx_ref, gW_ref = torch.zeros_like(to64(x)), torch.zeros_like(to64(W))
    O.backward_rgnn_relational_matmul(d, kind, to64(W).transpose(2, 3).contiguous(), to64(x), to64(go), gx_ref, gW_ref, in1head)
    gx, gW = torch.zeros_like(x, device=DEV), torch.zeros_like(W, device=DEV)
    K.backward_rgnn_relational_matmul(T._dev(d), kind, W.transpose(2, 3).contiguous().to(DEV), x.to(DEV), go.to(DEV), gx, gW, in1head)
    assert_close(gx, gx_ref, what="grad_x")
    assert_close(gW, gW_ref, what="grad_W")


@pytest.mark.parametrize("H,Kd,D,gather", [(4, 64, 16, False), (4, 64, 16, True), (1, 32, 32, False), (2, 64, 64, True), (4, 128, 32, False),
                                           (1, 32, 64, True)])
def test_rows_matmul_backward_dw_row_ladder(H, Kd, D, gather):
    """het_rows_matmul_backward_dw(_colsum) with the row-count ladder as its relations."""
    import het_amd.kernels as k
    rp = row_ladder_ptrs()
    R, n = rp.numel() - 1, int(rp[-1])
    gen = torch.Generator().manual_seed(Kd + D)
    X, Nx = H * D, n + 17
    x, go = torch.randn(Nx, Kd, generator=gen), torch.randn(n, X, generator=gen)
    idx = torch.randint(0, Nx, (n,), generator=gen) if gather else None
    gw, gw2, cs = (torch.full((R, H, Kd, D), 7.0, device=DEV), torch.full((R, H, Kd, D), 7.0, device=DEV), torch.full((X,), 7.0, device=DEV))
    xd = x.to(DEV) if gather else x[:n].to(DEV)
    idxd = None if idx is None else idx.to(DEV)
    k.rows_matmul_backward_dw(rp.to(DEV), idxd, xd, go.to(DEV), gw, accumulate=False, colsum=cs)
    k.rows_matmul_backward_dw(rp.to(DEV), idxd, xd, go.to(DEV), gw2, accumulate=False)
    assert_close(cs, go.double().sum(0), what="colsum")
    xs = (x[idx] if gather else x[:n]).double()
    for r in range(R):
        a, b = int(rp[r]), int(rp[r + 1])
        ref = (xs[a:b].t() @ go[a:b].double()).view(Kd, H, D).permute(1, 0, 2)
        assert_close(gw[r], ref, what=f"grad_w[{r}] ({b - a} rows)")
        assert_close(gw2[r], ref, what=f"grad_w[{r}] ({b - a} rows) without the sums")


# ---------------------------------------------------------------- relation-count ladder through the layers
R_LADDER = [1, 7, 8, 9, 12]


def _layer_graph(R):
    g = ladder_graph(R=R, seed=5, shuffle=False)  # (layers run on canonical eids, as HetGraph builds them)
    assert_rungs(ladder_counts(g)["in_rel"], LADDER, "in-degree per (relation, destination)")
    return g


@pytest.mark.parametrize("compact,direct,mulfirst", [(False, False, False), (True, True, False), (False, False, True)])
@pytest.mark.parametrize("R", R_LADDER)
def test_rgat_layer_relation_count(R, compact, direct, mulfirst):
    from tests.test_gpu_layers import _run_rgat
    _run_rgat(_layer_graph(R), H=4, K=64, X=64, compact=compact, direct=direct, mulfirst=mulfirst)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("R", R_LADDER)
def test_rgcn_layer_relation_count(R, compact):
    from tests.test_gpu_layers import _run_rgcn
    _run_rgcn(_layer_graph(R), compact, compact, 64, 64, R)


@pytest.mark.parametrize("R", R_LADDER)
def test_hgt_layer_relation_count(R, monkeypatch):
    from tests.test_gpu_layers import _run_hgt_fused
    _run_hgt_fused(False, True, 4, 64, 64, monkeypatch, g=_layer_graph(R))


# ---------------------------------------------------------------- moved thresholds (read once per process: a child interpreter)
@pytest.mark.parametrize("env", [{"HET_RGAT_HUB_MIN": "64"}, {"HET_RGAT_HUB_MIN": "384"}, {"HET_RGAT_BWD_PACK_T": "32"},
                                 {"HET_RGAT_BWD_PACK_T": "256"}], ids=["hub64", "hub384", "bwdpack32", "bwdpack256"])
def test_rgat_ladder_at_moved_thresholds(env):
    """The RGAT ladder cases with the hub threshold at 64 / 384 (384: destinations of more than HET_ITEM_MAX in-edges that are not
    hubs, walked whole by one lane group) and the backward's pack threshold at 32 / 256: each moves a threshold onto another rung."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_thresholds.py"), "-q", "-x", "-m", "gpu", "-k",
                        "test_rgat_ladder_run_sums or test_rgat_ladder_compact_passes", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
