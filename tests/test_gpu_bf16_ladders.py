"""The bf16 row entries, each on its own, on the two ladders of tests/util.py: ladder_graph (segments of exactly 32 / 64 / 256 / 257
edges, hubs of 513, destinations split over relations) for the gather passes and the node-major passes, ROW_LADDER (relations of 0, 1,
31 .. 33, 63 .. 65, 2047 .. 2049 and 4097 rows, boundaries mid-tile and mid-chunk) for the dense row kernels.  A bf16 row has 8
elements per 16 bytes where an fp32 row has 4: lanes per row, rows per step, tail masks and store paths are not the fp32 instances'.

Every case: bf16 inputs drawn in fp32 and rounded once, the fp64 reference evaluated on the rounded values (tests/_bf16_rows_ref.py,
held against the oracle and against deliberately wrong results in tests/test_bf16_rows_ref.py).  fp32 outputs: tests/util.py::
assert_close at its defaults (the bound the fp32 twins meet on the same lists).  bf16 outputs: elementwise |out - ref| <= 2^-8 |ref| +
A max|ref|.  Output buffers are pre-filled with NaN (7.0 where the entry accumulates or skips rows); rows an entry must not write are
checked for their old bits.

A = tests/_bf16_rows_ref.py::ABS_TERM = 1e-5: the fp32 CPU evaluation of each reference, rounded to bf16, needs 0 .. 2.8e-7 against the
fp64 one (tests/test_bf16_rows_ref.py prints the value of every case); times 4 (the project's margin for the GPU's summation order,
tests/test_gpu_rgat_bf16.py) that is below RGCN's 1e-5 (tests/test_gpu_rgcn_bf16.py::_check_bf16), which is the floor.

entry                                   test                                        ladder          shapes
rgat_aggregate_compact_bf16             test_rgat_gather_passes_*                   graph + hubs    (H, D) of RUN_SHAPES; D = 16 also with el from the row
rgat_aggregate_compact_forward_bf16     test_rgat_gather_passes_*                   graph + hubs    the same calls: equal bits with the training entry
rgat_backward_compact_bf16              test_rgat_gather_passes_*                   graph + hubs    the same; once without fold and bias
rgat_node_backward_dx_bf16              test_rgat_node_backward_dx_bf16_*           graph           (H, K, D): every <H*D, K / 32> instance
node_rows_matmul_sum_bf16               test_node_rows_matmul_sum_bf16_*            graph, R ladder R + 1 sources of 32 -> 32; 3 + 1 of every (KS, XO)
rows_matmul_bf16                        test_rows_matmul_bf16_row_ladder            rows            K in 32, 64 x X in 32, 64, 128; 4 list forms
rows_matmul_backward_dw_bf16            test_rows_matmul_backward_dw_bf16_row_ladder rows           the same (K, X); fp32 and bf16 gradout
rows_matmul_heads_bf16                  test_rows_matmul_heads_bf16_row_ladder      rows            every (K, H*D) of 32, 64, 128; heads of 16, 32, 64
rows_dot1h_bf16                         test_rows_dot1h_bf16_row_ladder             rows            H in 1, 2, 4, 8 x K in 32, 64
rows_dot1h_backward_dw_bf16             test_rows_dot1h_bf16_row_ladder             rows            the same; accumulate off and on
rgat_el_rows_bf16                       test_rgat_el_rows_bf16_row_ladder           rows            (H, D) of RUN_SHAPES
rows_linear_bias_bf16                   test_rows_linear_bias_bf16_row_ladder       rows            K, X in 32, 64, 128; ranges = the ladder's relations
hgt_aggregate / backward_compact_bf16   test_hgt_bf16_ladder_compact_passes         graph           HGT_ROWS
rgcn_layer_forward / backward_bf16      test_rgcn_bf16_ladder_layer                 graph, R 3, 7   (64, 64), (32, 32)"""
import pytest
import torch

import tests.test_gpu_ops as T
from tests import _bf16_rows_ref as B
from tests.test_gpu_thresholds import HGT_ROWS, RUN_SHAPES
from tests.util import LADDER, ROW_LADDER, assert_ladder, assert_rungs, ladder_counts, ladder_graph, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F64 = torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ladder():
    g = ladder_graph(R=5, seed=0)
    assert_ladder(g)
    return g


@pytest.fixture(scope="module")
def hubs():
    return random_graph(seed=31, n=12, r=4, e=9000)  # several runs per hub destination


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


# ---------------------------------------------------------------- 1. RGAT training gather passes
def _aggregate(k, c, grp, fb, el_d, er_d, h_before, nh, **el_from_row):
    """One call of the training entry into fresh buffers: (dict for check_aggregate, runs)."""
    N, H, D = c.N, fb.shape[1], fb.shape[2]
    sm, ret, h = torch.full((N, H), 7.0, device=DEV), torch.full((N, H, D), 7.0, device=DEV), h_before.to(DEV)
    runs = k.rgat_aggregate_compact_bf16(grp, fb, el_d, er_d, sm, ret, c.slope, h[:nh], c.R, **el_from_row)
    return dict(sum=sm, ret=ret, q_rows=runs[0], q_sum=runs[1], q_ref=runs[2], h_inout=h, h_before=h_before), runs


def rgat_gather_passes_case(g, H, D, fold, bias):
    """The bf16 twin of tests/test_gpu_ops.py::rgat_run_sums_case: its row maps and oracle calls (rgat_run_sums_reference) on feat_c /
    gradout rounded to bf16 once.
      rgat_aggregate_compact_bf16: sum (log-sum-exp, exactly 0 without in-edges), ret, the three run sums (rescaled by exp(q_ref)),
        h_inout against h0 + ret_ref with nh = N - 2 -- rows beyond nh and rows without in-edges keep their bits.
      rgat_aggregate_compact_forward_bf16 on the same arguments: torch.equal with the training entry's h_inout on EVERY destination.
        csrc/gat_compact.hip shows the same summation order for all of them: the packed walks (HET_rgat_aggregate_runs_packed / _fwd)
        apply online_edge to the same edges in the same order and end in acc * rcp(sum) added to h0 as a rounded product and a rounded
        sum (add_mul_rounded in the forward instance); the hub items and the hub finish (HET_rgat_aggregate_hub_items / _fwd,
        HET_rgat_finish_hubs / _fwd) are statement-for-statement copies for O, max and sum, and both divide with 1.f / ts.  So there
        is no "rest" to put under the elementwise bound.
      D = 16: the same with el_c = <feat_c, attn_l[r]> gathered, and formed from the gathered row (attn_l + feat_rel_ptrs; the el_c
        handed over is NaN, the forward-only entry gets none) -- both against the fp64 reference of that el.
      rgat_backward_compact_bf16 (bf16 gradout): grad_feat_c (with the fold), grad_el_c, grad_er_c, grad_bias over N - 3 rows and
        grad_attn_l -- or none of the last two and no fold."""
    import het_amd.kernels as k
    assert k.rgat_runs_shape_ok(H, D) and k.rgat_bf16_shape_ok(H, 64, D)
    c = T.rgat_run_sums_reference(g, H, D, fold, rows=B.bf16_round)
    grp = T.rgat_run_sums_groupings(c)
    N, R, nh, nb = c.N, c.R, c.N - 2, c.N - 3
    h0 = B.bf16_input(nh, H * D, gen=c.gen)
    h_before = torch.full((N, H * D), 3.0, dtype=BF16)
    h_before[:nh] = h0
    ref = dict(has_in=c.has_in, nh=nh, lse=torch.where(c.has_in.unsqueeze(-1), torch.log(c.sm_r), torch.zeros_like(c.sm_r)), ret=c.ret_r,
               q_sum=c.q_ref, q_rows=c.Q_ref, h_ref=h0.double() + c.ret_r.view(N, -1)[:nh])
    fb, gob, el_d, er_d = c.feat.to(BF16).to(DEV), c.go.to(BF16).to(DEV), c.el.to(DEV), c.er.to(DEV)
    assert torch.equal(fb.float().cpu(), c.feat) and torch.equal(gob.float().cpu(), c.go)  # (rounded once, before the reference)
    got, runs = _aggregate(k, c, grp, fb, el_d, er_d, h_before, nh)
    B.check_aggregate("rgat_aggregate_compact_bf16", got, ref)
    hf = h_before.to(DEV)
    k.rgat_aggregate_compact_forward_bf16(grp, fb, el_d, er_d, hf[:nh], c.slope, R)
    assert torch.equal(hf, got["h_inout"]), "rgat_aggregate_compact_forward_bf16: not the rows the training entry stores"
    if D == 16:
        assert k.rgat_el_from_row(H, D, R)
        el2 = (c.feat.double() * c.attn.double()[c.rel_of_row]).sum(-1)
        r2 = B.rgat_runs_reference(c.feat.double(), el2, c.er.double(), c.go.double(), c.srow_p, c.drow_p, c.s["col_indices"], N, c.slope,
                                   h0=h0.double())
        r2["nh"] = nh
        rowp = dict(attn_l=_d(c.attn), feat_rel_ptrs=_d(c.ss["rel_ptrs_row"]))
        gA, _ = _aggregate(k, c, grp, fb, _d(el2.float()), er_d, h_before, nh)
        gB, _ = _aggregate(k, c, grp, fb, torch.full_like(el_d, NAN), er_d, h_before, nh, **rowp)
        B.check_aggregate("rgat_aggregate_compact_bf16 (el = <feat, attn_l>, gathered)", gA, r2)
        B.check_aggregate("rgat_aggregate_compact_bf16 (el from the row)", gB, r2)
        hf = h_before.to(DEV)
        k.rgat_aggregate_compact_forward_bf16(grp, fb, None, er_d, hf[:nh], c.slope, R, **rowp)
        assert torch.equal(hf, gB["h_inout"]), "rgat_aggregate_compact_forward_bf16 (el from the row): not the training entry's rows"
    gf, gl, gr = (torch.full((c.S_row, H, D), NAN, device=DEV), torch.full((c.S_row, H), NAN, device=DEV), torch.full((c.S_col, H), NAN, device=DEV))
    gb = torch.full((H * D,), NAN, device=DEV) if bias else None
    ga = torch.full((R, H, D), NAN, device=DEV) if fold else None
    k.rgat_backward_compact_bf16(grp, fb, el_d, er_d, got["sum"], got["ret"], gob, gf, gl, gr, c.slope, runs, _d(c.ss["node_indices_col"]),
                                 fold_attn_l=_d(c.attn) if fold else None, row_rel_ptrs=_d(c.ss["rel_ptrs_row"]) if fold else None,
                                 grad_bias=gb, bias_rows=nb, grad_attn_l=ga)
    B.check_backward("rgat_backward_compact_bf16", dict(grad_feat=gf, grad_el=gl, grad_er=gr, grad_bias=gb, grad_attn_l=ga),
                     dict(grad_feat=c.gf_r, grad_el=c.gl_r, grad_er=c.gr_r, grad_bias=c.go.double().view(N, -1)[:nb].sum(0) if bias else None,
                          grad_attn_l=c.ga_r if fold else None))


@pytest.mark.parametrize("H,D", RUN_SHAPES)
def test_rgat_gather_passes_ladder(ladder, H, D):
    """Every (lanes per row, lanes per head) pair of HET_DISPATCH_COOP -- rows of 32 / 64 / 128 elements, heads of 16 .. 128 -- and,
    at D = 16, the el-from-the-row instances (LPR 8 / 16 / 32, DL 4), on the degree ladder: packs, runs of exactly 32 / 64 / 256 / 257,
    hubs of 513, destinations split over relations, an empty relation, nodes without edges."""
    rgat_gather_passes_case(ladder, H, D, fold=True, bias=True)


@pytest.mark.parametrize("H,D", RUN_SHAPES)
def test_rgat_gather_passes_hubs(hubs, H, D):
    """12 destinations of ~750 in-edges: every destination a hub of several runs, each run of several work items."""
    rgat_gather_passes_case(hubs, H, D, fold=True, bias=True)


def test_rgat_gather_passes_ladder_without_fold(ladder):
    rgat_gather_passes_case(ladder, 4, 16, fold=False, bias=False)


def test_rgat_gather_passes_refuse_other_shapes(ladder):
    """Heads of 8 (LPR_SHAPES of the fp32 ladder) are outside the run-sum form: refused, nothing written."""
    import het_amd.kernels as k
    from het_amd import _lib
    H, D = 8, 8
    assert not k.rgat_runs_shape_ok(H, D) and not k.rgat_bf16_shape_ok(H, 64, D)
    c = T.rgat_run_sums_reference(ladder, H, D, False, rows=B.bf16_round)
    grp = T.rgat_run_sums_groupings(c)
    fb, h = c.feat.to(BF16).to(DEV), torch.full((c.N, H * D), 3.0, dtype=BF16, device=DEV)
    sm, ret = torch.full((c.N, H), 7.0, device=DEV), torch.full((c.N, H, D), 7.0, device=DEV)
    with pytest.raises(_lib.HetError):
        k.rgat_aggregate_compact_bf16(grp, fb, _d(c.el), _d(c.er), sm, ret, c.slope, h, c.R)
    with pytest.raises(_lib.HetError):
        k.rgat_aggregate_compact_forward_bf16(grp, fb, _d(c.el), _d(c.er), h, c.slope, c.R)
    torch.cuda.synchronize()
    assert bool((h == 3.0).all()) and bool((sm == 7.0).all()) and bool((ret == 7.0).all())


# ---------------------------------------------------------------- 2. node-major input gradient
# test_rgat_node_backward_dx_ladder's list -- HET_node_dx<64, 2> (4 waves: the 1 + R weights of 64 x 64 fill the LDS) and <32, 1> (8 waves)
# -- and the two mixed instances <64, 1> (K = 32 from rows of 64) and <32, 2> (K = 64 from rows of 32)
NODE_DX_SHAPES = B.NODE_DX_SHAPES + [(4, 32, 16), (2, 64, 16)]


def _node_dx(k, c, node_order=None, n_begin=0, n_end=None):
    f = lambda t: None if t is None else t.float().to(DEV).contiguous()  # noqa: E731
    row_map, dst_map = k.node_row_map(_d(c.rp_row), _d(c.n_row), c.N), k.node_row_map(_d(c.rp_col), _d(c.n_col), c.N)
    out = torch.full((c.N, c.K), NAN, device=DEV, dtype=BF16)
    k.rgat_node_backward_dx_bf16(n_begin, c.N if n_end is None else n_end, c.n_loop, _d(c.gh), f(c.loop_w.t()) if c.gh is not None else None,
                                 f(c.g_rows), f(c.W.transpose(2, 3)), row_map, f(c.g_er), f(c.wa), dst_map, out, node_order)
    return out


@pytest.mark.parametrize("H,Kd,D", NODE_DX_SHAPES)
def test_rgat_node_backward_dx_bf16_ladder(ladder, H, Kd, D):
    """het_rgat_node_backward_dx_bf16 on the ladder's (relation, source) / (relation, destination) lists against the per-term sum:
    grad_h bf16, g_rows / g_er / weights fp32, grad_x bf16 rounded once; n_loop = N - 5.  Nodes without a row in any relation get the
    self-loop term alone, or -- beyond n_loop -- exactly zero."""
    import het_amd.kernels as k
    assert k.rgat_node_gemm_ok(ladder.get_num_rels(), H, Kd, D)
    c = B.node_dx_case(ladder, H, Kd, D)
    assert int(c.zero_rows.sum()) >= 1 and int((c.no_rows & ~c.zero_rows).sum()) >= 1
    B.check_node_dx("grad_x", _node_dx(k, c), B.node_dx_ref(c, F64), c.zero_rows)


def test_rgat_node_backward_dx_bf16_without_self_loop(ladder):
    """grad_h / loop_wt None: the relation terms alone; every node without a row is exactly zero."""
    import het_amd.kernels as k
    c = B.node_dx_case(ladder, 4, 64, 16, self_loop=False)
    assert bool((c.zero_rows == c.no_rows).all()) and int(c.zero_rows.sum()) >= 7
    B.check_node_dx("grad_x", _node_dx(k, c), B.node_dx_ref(c, F64), c.zero_rows)


def test_rgat_node_backward_dx_bf16_node_order(ladder):
    """node_order a random permutation: the same rows; and a sub-range [37, N - 11) of it: the nodes at the other positions keep
    their bits."""
    import het_amd.kernels as k
    c = B.node_dx_case(ladder, 2, 64, 32)
    ref = B.node_dx_ref(c, F64)
    perm = torch.randperm(c.N, generator=torch.Generator().manual_seed(9))
    order = perm.to(torch.int32).to(DEV)
    B.check_node_dx("grad_x (permuted)", _node_dx(k, c, order), ref, c.zero_rows)
    out = _node_dx(k, c, order, 37, c.N - 11)
    inside = torch.zeros(c.N, dtype=torch.bool)
    inside[perm[37:c.N - 11]] = True
    B.check_node_dx("grad_x (range of a permutation)", out[inside.to(DEV)], ref[inside], c.zero_rows[inside])
    B.check_same_bits("grad_x outside the range", out, torch.full((c.N, c.K), NAN, device=DEV, dtype=BF16), ~inside)


def _node_sum(k, c):
    row_map = k.node_row_map(_d(c.rp), _d(c.nodes), c.N)
    assert torch.equal(row_map.cpu().long(), c.maps)
    rd = _d(c.rows)
    sources = [(rd, 0, row_map[r].contiguous(), _d(c.wts[r])) for r in range(c.R)] + [(_d(c.xl), 0, None, _d(c.wts[c.R]))]
    out = torch.full((c.N, c.XO), NAN, device=DEV, dtype=BF16)
    k.node_rows_matmul_sum_bf16(0, c.N, sources, out)
    return out


@pytest.mark.parametrize("R", [1, 7, 8, 9, 12])
def test_node_rows_matmul_sum_bf16_relation_count(R):
    """The bf16 twin of test_node_rows_matmul_sum_relation_count: one source per relation + one identity-mapped source, up to
    kMaxSrc = 9 sources of 32 -> 32 (HET_node_rows_sum<32, 1>); more are refused by node_rows_matmul_sum_ok and by the entry."""
    import het_amd.kernels as k
    from het_amd import _lib
    c = B.node_sum_case(ladder_graph(R=R, seed=4, shuffle=False), 32, 32, R)
    assert k.node_rows_matmul_sum_ok(R + 1, 32, 32) == (R + 1 <= 9)
    if R + 1 > 9:
        with pytest.raises(_lib.HetError):
            _node_sum(k, c)
        return
    B.check_bf16(f"node sum of {R + 1} sources", _node_sum(k, c), B.node_sum_ref(c, F64))


@pytest.mark.parametrize("KS,XO", B.NODE_SUM_WIDTHS)
def test_node_rows_matmul_sum_bf16_widths(KS, XO):
    """HET_node_rows_sum<32, 2>, <64, 1> and <64, 2> with 3 + 1 sources on the ladder graph."""
    import het_amd.kernels as k
    c = B.node_sum_case(ladder_graph(R=3, seed=4, shuffle=False), KS, XO, 3)
    assert k.node_rows_matmul_sum_ok(4, KS, XO)
    B.check_bf16(f"node sum {KS} -> {XO}", _node_sum(k, c), B.node_sum_ref(c, F64))


# ---------------------------------------------------------------- 3. dense bf16 row kernels on the row-count ladder
@pytest.mark.parametrize("K,X", B.ROWS_MATMUL_SHAPES)
def test_rows_matmul_bf16_row_ladder(K, X):
    """het_rows_matmul_bf16: HET_seg_gemm_mfma<K, NT, .., het_bf16, het_bf16> with K in 32, 64 and NT = X / 32 in 1, 2; X = 128 runs as
    two 64-wide column slabs of NT = 2.  Without lists, with a gather list (repeats), with a scatter list (distinct rows) and with
    both; rows the scatter list does not name, and rows beyond the list, keep their bits."""
    import het_amd.kernels as k
    assert k.rows_matmul_bf16_ok(K, X)
    c = B.dense_case(K, X, seed=K + X)
    rp, xd, W = _d(c.rp), _d(c.x), _d(c.W.view(c.R, 1, K, X))
    for gather in (False, True):
        ref = B.rows_matmul_ref(c, F64, gather)
        for scatter in (False, True):
            before = torch.full((c.No, X), NAN, dtype=BF16)
            out = before.to(DEV)
            # (without lists the row count is x's: its first n rows)
            k.rows_matmul_bf16(rp, _d(c.gather) if gather else None, _d(c.scatter) if scatter else None, W, xd if gather else xd[:c.n], out)
            rows = c.scatter if scatter else torch.arange(c.n)
            B.check_bf16(f"out (gather={gather}, scatter={scatter})", out[rows.to(DEV)], ref)
            written = torch.zeros(c.No, dtype=torch.bool)
            written[rows] = True
            B.check_same_bits(f"out (gather={gather}, scatter={scatter})", out, before, ~written)


@pytest.mark.parametrize("bf16_gradout", [False, True], ids=["gradout_fp32", "gradout_bf16"])
@pytest.mark.parametrize("K,X", B.ROWS_MATMUL_SHAPES)
def test_rows_matmul_backward_dw_bf16_row_ladder(K, X, bf16_gradout):
    """het_rows_matmul_backward_dw_bf16 (fp32 gradout, row i) / _bf16_bf16 (bf16 gradout through g_rows): HET_seg_dw_mfma<KT, NT> with
    KT = K / 32 and NT in 1, 2 (X = 128: two blocks along blockIdx.y), chunks of 512 rows -- the 2047 / 2048 / 2049 / 4097-row
    relations span several workgroups that meet in float atomics.  accumulate off (onto 7.0) and on (onto a non-zero grad_w)."""
    import het_amd.kernels as k
    c = B.dense_case(K, X, seed=K + X)
    rp, xd, idx = _d(c.rp), _d(c.x), _d(c.gather)
    go, g_rows = (_d(c.gob), _d(c.g_rows)) if bf16_gradout else (_d(c.go32[:c.n]), None)
    for accumulate in (False, True):
        gw = _d(c.gw0.view(c.R, 1, K, X)) if accumulate else torch.full((c.R, 1, K, X), 7.0, device=DEV)
        k.rows_matmul_backward_dw_bf16(rp, idx, xd, go, gw, accumulate, g_rows=g_rows)
        B.check_per_relation(f"grad_w (accumulate={accumulate})", gw.view(c.R, K, X), B.rows_matmul_dw_ref(c, F64, True, bf16_gradout, accumulate),
                             c.rp)


@pytest.mark.parametrize("H,K,D", B.HEADS_SHAPES)
def test_rows_matmul_heads_bf16_row_ladder(H, K, D):
    """het_rows_matmul_heads_bf16: the same kernel with the head-concatenated weight [R,H,K,D] -- every (K, H*D) pair of 32 / 64 / 128
    (launch_kx<K, 1 or 2>; H*D = 128 as two slabs that start inside the head layout), heads of 16, 32 and 64."""
    import het_amd.kernels as k
    c = B.heads_case(H, K, D, seed=H + K + D)
    out = torch.full((c.n, H, D), NAN, device=DEV, dtype=BF16)
    k.rows_matmul_heads_bf16(_d(c.rp), _d(c.gather), _d(c.W), _d(c.x), out)
    B.check_bf16("feat_c", out.view(c.n, H * D), B.heads_ref(c, F64))


@pytest.mark.parametrize("H,K", B.DOT1H_SHAPES)
def test_rows_dot1h_bf16_row_ladder(H, K):
    """het_rows_dot1h_bf16 (HET_rowdot1h_fwd_bf16<K / 4, H>) and its weight gradient het_rows_dot1h_backward_dw_bf16
    (HET_rowdot1h_bwd_dw_bf16<K / 4, H>: chunks of kDwMinChunk = 512 rows, so the 2047 / 2048 / 2049 / 4097-row relations take several
    workgroups, tile_to_relation meets relation boundaries mid-chunk and the partial rows meet in atomic_add4): H in 1, 2, 4, 8 (one
    16-byte load of the H gradients at H = 4), K in 32, 64.  Reference: SUM_i gradout[i,h] x[idx[i]] per relation in fp64."""
    import het_amd.kernels as k
    c = B.dense_case(K, 32, seed=7 * H + K, H=H)
    rp, xd, idx = _d(c.rp), _d(c.x), _d(c.gather)
    out = torch.full((c.n, H), NAN, device=DEV)
    k.rows_dot1h_bf16(rp, idx, _d(c.w1h), xd, out)
    B.check_f32("er_c", out, B.rows_dot1h_ref(c, F64))
    for accumulate in (False, True):
        gw = _d(c.gw1h0) if accumulate else torch.full((c.R, H, K), 7.0, device=DEV)
        k.rows_dot1h_backward_dw_bf16(rp, idx, xd, _d(c.go1h), gw, accumulate)
        B.check_per_relation(f"grad_w (accumulate={accumulate})", gw, B.rows_dot1h_dw_ref(c, F64, accumulate), c.rp)


@pytest.mark.parametrize("H,D", B.EL_ROWS_SHAPES)
def test_rgat_el_rows_bf16_row_ladder(H, D):
    """het_rgat_el_rows_bf16 (HET_rgat_el_rows_bf16<H*D / 4>: a lane group per row, 64 / LPR rows per wave): rows of 32 / 64 / 128 with
    heads of 16 .. 128, the relation of a row found from rel_ptrs."""
    import het_amd.kernels as k
    c = B.el_rows_case(H, D, seed=H + D)
    el = torch.full((c.n, H), NAN, device=DEV)
    k.rgat_el_rows_bf16(_d(c.rp), _d(c.feat), _d(c.attn), el)
    B.check_f32("el_c", el, B.el_rows_ref(c, F64))


def test_dense_entries_refuse_other_shapes():
    """Shapes outside an entry's dispatch are refused with HET_ERR_UNSUPPORTED (code 3) and nothing is written: heads of 8 for
    rgat_el_rows_bf16, K = 128 for rows_matmul_bf16 and its weight gradient, K = 16 for rows_matmul_heads_bf16 and
    rows_linear_bias_bf16, K < 4 H for the one-head row-dot pair."""
    import het_amd.kernels as k
    from het_amd import _lib
    unsupported = pytest.raises(_lib.HetError, match="code 3")
    c = B.el_rows_case(8, 8, seed=1)
    el = torch.full((c.n, 8), 7.0, device=DEV)
    with unsupported:
        k.rgat_el_rows_bf16(_d(c.rp), _d(c.feat), _d(c.attn), el)
    assert not k.rows_matmul_bf16_ok(128, 64) and not k.rows_linear_bias_ok(16, 32)
    c = B.dense_case(128, 64, seed=2)
    out, gw = torch.full((c.No, 64), 7.0, device=DEV, dtype=BF16), torch.full((c.R, 1, 128, 64), 7.0, device=DEV)
    with unsupported:
        k.rows_matmul_bf16(_d(c.rp), _d(c.gather), None, _d(c.W.view(c.R, 1, 128, 64)), _d(c.x), out)
    with unsupported:
        k.rows_matmul_backward_dw_bf16(_d(c.rp), _d(c.gather), _d(c.x), _d(c.go32[:c.n]), gw, False)
    c = B.dense_case(16, 32, seed=3, H=8)
    out16, er, gw1 = torch.full((c.Nx, 32), 7.0, device=DEV, dtype=BF16), torch.full((c.n, 8), 7.0, device=DEV), torch.full((c.R, 8, 16), 7.0, device=DEV)
    with unsupported:
        k.rows_linear_bias_bf16(_d(c.rp[:2].clone()), _d(c.x), _d(c.W[0]), None, out16)
    with unsupported:
        k.rows_dot1h_bf16(_d(c.rp), _d(c.gather), _d(c.w1h), _d(c.x), er)
    with unsupported:
        k.rows_dot1h_backward_dw_bf16(_d(c.rp), _d(c.gather), _d(c.x), _d(c.go1h), gw1, False)
    h = B.heads_case(2, 16, 16, seed=4)
    feat = torch.full((h.n, 2, 16), 7.0, device=DEV, dtype=BF16)
    with unsupported:
        k.rows_matmul_heads_bf16(_d(h.rp), _d(h.gather), _d(h.W), _d(h.x), feat)
    torch.cuda.synchronize()
    for t in (el, out, gw, out16, er, gw1, feat):
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K,X", B.LINEAR_SHAPES)
def test_rows_linear_bias_bf16_row_ladder(K, X, bias):
    """het_rows_linear_bias_bf16 (the same kernel with one segment and the bias epilogue; launch_kx<32 / 64 / 128, 1 or 2>, X = 128 as
    two slabs with the bias moved along): the row range [offsets[0], offsets[1]) set to every relation of the row ladder in turn --
    node-type offsets with their boundaries at the ladder counts --; after each call the rows outside the range hold their old bits."""
    import het_amd.kernels as k
    assert k.rows_linear_bias_ok(K, X)
    c = B.dense_case(K, X, seed=3 * K + X)
    ref = B.linear_bias_ref(c, F64, bias)
    xd, w, b = _d(c.x), _d(c.W[0]), _d(c.bias) if bias else None
    out = torch.full((c.Nx, X), NAN, device=DEV, dtype=BF16)
    rows = torch.arange(c.Nx)
    for r in range(c.R):
        lo, hi = int(c.rp[r]), int(c.rp[r + 1])
        before = out.clone()
        assert k.rows_linear_bias_bf16(_d(c.rp[r:r + 2].clone()), xd, w, b, out) is out
        B.check_bf16(f"rows [{lo}, {hi}) ({hi - lo} rows)", out[lo:hi], ref[lo:hi])
        B.check_same_bits(f"rows outside [{lo}, {hi})", out, before, (rows < lo) | (rows >= hi))
    B.check_bf16("all rows of the ladder", out[:c.n], ref[:c.n])
    assert bool(torch.isnan(out[c.n:].float()).all())


# ---------------------------------------------------------------- 4. the two neighbours
@pytest.mark.parametrize("H,D", HGT_ROWS)
def test_hgt_bf16_ladder_compact_passes(ladder, H, D):
    """tests/test_gpu_hgt_bf16.py::_op_case (elementwise bf16 bound for out, fp32 bound for lsum and both gradients) on the degree
    ladder, for every (lanes per row, lanes per head) pair of HET_DISPATCH_HGT_ROWS -- the bf16 entries take them all."""
    import het_amd.kernels as k
    from tests.test_gpu_hgt_bf16 import _op_case
    assert k.hgt_compact_shape_ok(H, D)
    _op_case(ladder, H, D)


@pytest.mark.parametrize("Kd,D", [(64, 64), (32, 32)])
@pytest.mark.parametrize("R", [3, 7])
def test_rgcn_bf16_ladder_layer(R, Kd, D):
    """tests/test_gpu_rgcn_bf16.py::_bf16_step (elementwise bf16 bound for out and grad_x, 1e-5 relative L2 for grad_W and grad_bias) on
    the degree ladder with 3 and 7 relations."""
    import het_amd.kernels as k
    from tests.test_gpu_rgcn_bf16 import _bf16_step
    g = ladder_graph(R=R, seed=6)
    assert_rungs(ladder_counts(g)["in_rel"], LADDER, "in-degree per (relation, destination)")
    assert k.rgcn_layer_ok(R, Kd, D)
    _bf16_step(g, Kd, D, R)


def test_row_ladder_is_what_the_docstrings_say():
    assert sorted(ROW_LADDER) == [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097] and sum(ROW_LADDER) == 10530
