"""Shared helpers of the GPU parity tests."""
import torch

from het_amd.graph import HetGraph
from het_amd.synth import make_mag_like, make_random


def cpu(t):
    return t.detach().cpu()


def to64(t):
    return t.detach().cpu().double()


def random_graph(seed=0, n=257, r=5, e=3001, empty_rel=True, shuffle=True):
    coo = make_random(n, r, e, seed=seed)
    if empty_rel and r > 2:  # leave one relation empty, one tiny
        coo.rel[coo.rel == 1] = 0
        coo.rel = torch.sort(coo.rel).values
    g = HetGraph.from_integrated_coo(coo)
    if shuffle:
        permute_eids(g, seed + 1000)
    return g


def permute_eids(g, seed):
    """HetGraph canonicalises eids to arange(E) in separate-COO order, as the reference does; the ops accept any
    edge numbering, so renumber every layout's eids with one random permutation (edge data row != position)."""
    E = g.get_num_edges()
    pi = torch.randperm(E, generator=torch.Generator().manual_seed(seed))

    def walk(d):
        for k, v in d.items():
            if isinstance(v, dict):
                walk(v)
            elif k == "eids":
                d[k] = pi[v]
            elif k in ("inverse_indices_row", "inverse_indices_col") and v.numel() == E:
                # the single-sided inverse indices are read by EDGE ID (inverse_indices_row[eid] = compact row of that edge's
                # source: SURVEY.md section 9, layouts table): the entry of position p moves to the position's new id
                moved = torch.empty_like(v)
                moved[pi] = v
                d[k] = moved

    walk(g.graph_data)
    g._plans.clear()


# Counts at which the grouped kernels change code path (HET_PACK_T = 32, the RGAT backward's pack threshold 64, HET_ITEM_MAX = 256, the
# RGAT hub threshold 256, the edges per unrolled step of the gather loops) and the counts on either side of them.
LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 769)
# destinations whose in-edges are split over several relations: (destination total, runs per relation)
LADDER_SPLITS = ((256, (128, 128)), (256, (100, 100, 56)), (256, (64, 64, 64, 64)),   # a total of exactly 256, every run shorter
                 (257, (129, 128)), (257, (86, 86, 85)), (257, (65, 64, 64, 64)),     # 257: a hub made of short runs only
                 (400, (300, 100)), (523, (513, 10)),                                  # a hub with a run longer than one work item
                 (32, (16, 16)), (33, (17, 16)), (64, (32, 32)), (65, (33, 32)), (65, (20, 20, 25)))
# rows per relation of the segment GEMMs (32-row MFMA tiles, 64-row tiles, 2048-row chunks), in an order that puts the relation
# boundaries mid-tile
ROW_LADDER = (1, 31, 0, 33, 2047, 32, 65, 2048, 63, 4097, 64, 2049)


def ladder_graph(R=5, seed=0, shuffle=True, pool=3000, isolated=7):
    """A HetGraph whose counts take every value of LADDER exactly, each independently of the others:
      * in-degree per (relation, destination): one destination per rung, all its in-edges in one relation (so the destination
        total is the rung too: single runs of 257 / 513 make hubs whose only run spans several work items);
      * destinations whose in-edges split over several relations (LADDER_SPLITS);
      * out-degree per (relation, source): one source per rung, in one relation.
    The destination rungs take their sources from a pool of `pool` nodes, the source rungs their destinations from the same pool,
    so that the pool's own counts stay small and no rung is disturbed.  Relation 2 is left empty (R >= 4), the last `isolated`
    nodes have no edges, and with `shuffle` the eids are a random permutation.  With R < 4 the splits fold onto fewer relations
    (runs of one relation merge); the rungs above stay exact.  About 11 000 edges."""
    from het_amd.synth import IntegratedCOO
    gen = torch.Generator().manual_seed(seed)
    rels = [r for r in range(R) if not (R >= 4 and r == 2)]  # the relations that get edges
    n_dst = len(LADDER) + len(LADDER_SPLITS)
    dst0, src0 = 0, n_dst
    pool0 = src0 + len(LADDER)
    N = pool0 + pool + isolated
    rows, cols, rtype = [], [], []

    def add(src, dst, r):
        rows.append(src)
        cols.append(dst)
        rtype.append(torch.full((src.numel(),), r, dtype=torch.int64))

    for i, c in enumerate(LADDER):  # destination rungs (sources from the pool)
        add(pool0 + torch.randint(0, pool, (c,), generator=gen), torch.full((c,), dst0 + i), rels[i % len(rels)])
    for i, (total, runs) in enumerate(LADDER_SPLITS):
        assert sum(runs) == total
        v = dst0 + len(LADDER) + i
        for j, c in enumerate(runs):
            add(pool0 + torch.randint(0, pool, (c,), generator=gen), torch.full((c,), v), rels[(i + j) % len(rels)])
    for i, c in enumerate(LADDER):  # source rungs (destinations from the pool)
        add(torch.full((c,), src0 + i), pool0 + torch.randint(0, pool, (c,), generator=gen), rels[(i + 1) % len(rels)])
    row, col, rel = torch.cat(rows), torch.cat(cols), torch.cat(rtype)
    o = torch.randperm(row.numel(), generator=gen)  # edges of a relation in no particular order
    row, col, rel = row[o], col[o], rel[o]
    o = torch.sort(rel, stable=True).indices
    coo = IntegratedCOO(N, R, torch.tensor([0, N]), row[o], col[o], rel[o], torch.arange(row.numel(), dtype=torch.int64))
    g = HetGraph.from_integrated_coo(coo)
    if shuffle:
        permute_eids(g, seed + 1000)
    return g


def ladder_counts(g):
    """The counts ladder_graph prescribes, as measured on a graph: {"in_rel": in-degree per (relation, destination), "in": per
    destination over all relations, "out_rel": out-degree per (relation, source), "rel": edges per relation} (zeros dropped but
    for "rel")."""
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    nz = lambda t: t[t > 0]  # noqa: E731
    return {"in_rel": nz(torch.bincount(rel * N + s["col_indices"], minlength=R * N)),
            "in": nz(torch.bincount(s["col_indices"], minlength=N)),
            "out_rel": nz(torch.bincount(rel * N + s["row_indices"], minlength=R * N)),
            "rel": s["rel_ptrs"][1:] - s["rel_ptrs"][:-1]}


def assert_rungs(counts, values, what=""):
    """Every value of `values` occurs in the histogram `counts`."""
    have = set(counts.tolist())
    missing = [v for v in values if v not in have]
    assert not missing, f"{what}: counts {missing} are not in the graph"


def assert_ladder(g):
    """The rungs of ladder_graph on `g` (R >= 4): every ladder count per (relation, destination), per destination and per
    (relation, source); the split destinations' totals; an empty relation; nodes without edges."""
    c = ladder_counts(g)
    assert_rungs(c["in_rel"], LADDER, "in-degree per (relation, destination)")
    assert_rungs(c["in"], LADDER + tuple(t for t, _ in LADDER_SPLITS), "in-degree per destination")
    assert_rungs(c["out_rel"], LADDER, "out-degree per (relation, source)")
    assert int((c["rel"] == 0).sum()) >= 1, "no empty relation"
    s = g.get_separate_coo_original()
    touched = torch.zeros(g.get_num_nodes(), dtype=torch.bool)
    touched[s["row_indices"]] = True
    touched[s["col_indices"]] = True
    assert not bool(touched.all()), "every node has an edge"


def row_ladder_ptrs():
    """Relation pointers [len(ROW_LADDER) + 1] of a row list whose relations have the ROW_LADDER row counts."""
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(ROW_LADDER, dtype=torch.int64), 0)])


def mag_graph(scale=2e-3):
    return HetGraph.from_integrated_coo(make_mag_like(scale=scale))


def assert_close(actual, expected, rtol=2e-4, atol=2e-5, what=""):
    """fp32 HIP result vs fp64 oracle.  Tolerance: the reference states rtol 1e-3 between
    implementations (hrt/python/utils_lite/graphiler_bench.py:22-26); we hold 2e-4, with atol
    scaled to the magnitude of the expected tensor (sums over up to thousands of edges)."""
    expected = expected.detach().to(torch.float64)
    scale = float(expected.abs().max()) if expected.numel() else 1.0
    torch.testing.assert_close(actual.detach().cpu().double(), expected, rtol=rtol, atol=atol * max(1.0, scale),
                               msg=lambda m: f"{what}: {m}")


def rgat_min_abs_preactivation(x, W, attn_l, attn_r, sep):
    """min |el + er| over the (edge, head) pairs of an RGAT layer, in fp64.  A pre-activation within fp32 rounding of 0 sits
    on the leaky-ReLU kink: the fp32 kernels (the reference's included) and the fp64 oracle can then take different
    branches, which changes a gradient by a finite amount -- inherent to fp32, not an error of either side.  The layer
    tests nudge their random input until no edge sits there."""
    R = W.shape[0]
    rel = torch.repeat_interleave(torch.arange(R), sep["rel_ptrs"][1:] - sep["rel_ptrs"][:-1])
    x, W = x.double(), W.detach().double()
    wl = torch.einsum("rhkd,rhd->rhk", W, attn_l.detach().double())  # el = x[src] . (W . attn_l)
    wr = torch.einsum("rhkd,rhd->rhk", W, attn_r.detach().double())
    z = torch.einsum("ek,ehk->eh", x[sep["row_indices"]], wl[rel]) + torch.einsum("ek,ehk->eh", x[sep["col_indices"]], wr[rel])
    return float(z.abs().min()) if z.numel() else 1.0


def rgat_nudge_off_kink(x, W, attn_l, attn_r, sep, margin=2e-6, max_rounds=40, step=1e-3, seed=0):
    """x with the rows of a few nodes moved by ~`step` so that no (edge, head) pre-activation el + er (fp64) lies within
    `margin` of the leaky-ReLU kink; returns (x, min |el + er|).  Works on any device and at full size: with 84 M
    pre-activations a few hundred land within 2e-6 of zero whatever the seed, so re-drawing the whole input cannot clear
    them -- instead only ONE endpoint of every offending edge is moved (the one that touches fewer edges), which re-draws
    the pre-activations of that node's edges only; a couple of rounds leave none."""
    R = W.shape[0]
    dev = x.device
    rp, row, col = sep["rel_ptrs"].to(dev), sep["row_indices"].to(dev), sep["col_indices"].to(dev)
    rel = torch.repeat_interleave(torch.arange(R, device=dev), rp[1:] - rp[:-1])
    W64 = W.detach().double()
    wl = torch.einsum("rhkd,rhd->rhk", W64, attn_l.detach().double())  # el = x[src] . (W . attn_l)
    wr = torch.einsum("rhkd,rhd->rhk", W64, attn_r.detach().double())
    N = x.shape[0]
    deg = torch.bincount(row, minlength=N) + torch.bincount(col, minlength=N)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = x.clone()
    zmin = 1.0
    for _ in range(max_rounds):
        x64 = x.double()
        el_n = torch.einsum("nk,rhk->rnh", x64, wl)  # [R, N, H]
        er_n = torch.einsum("nk,rhk->rnh", x64, wr)
        z = el_n[rel, row] + er_n[rel, col]           # [E, H]
        za = z.abs().min(dim=1).values
        zmin = float(za.min()) if za.numel() else 1.0
        bad = torch.nonzero(za < margin).flatten()
        del el_n, er_n, z, za
        if bad.numel() == 0:
            break
        s, d = row[bad], col[bad]
        move = torch.unique(torch.where(deg[s] <= deg[d], s, d))
        x[move] += step * torch.randn(move.numel(), x.shape[1], device=dev, generator=gen, dtype=x.dtype)
    return x, zmin


def check_round5_gat_pins(ops, dev, gold, lists, inputs, slope, rtol_exp=1e-6, atol_exp=1e-7, rtol_sum=1e-5, atol_sum=1e-6):
    """The round-5 golden vectors of tests/golden/make_golden.py (what the rest of the reference's ref_rgat.py can pin), held against
    ``ops`` -- the oracle module or ``torch.ops.torch_hrt`` -- on device ``dev``:
      kind 1 forward  exp / sum   (el / er on the two-sided unique list, rows found by search)         gatk1_exp, gatk1_sum
      kind 2 forward  sum         (both edge ends through ONE inverse index; the reference loses exp)  gatk2_sum
      kind 4 backward grad_feat   (compact rows summed per source node, as the reference indexes it)   gatcb_grad_feat_src
      kind 1 backward grad_feat   (same)                                                               gatk1b_grad_feat_src
    lists: sep_rel_ptrs / sep_row / sep_col, ts_rel_ptrs / ts_node_indices / ts_inverse_indices, ss_inverse_indices_row / _col,
    ss_node_indices_row (the reference builders' outputs, or ours on the same graph -- they are equal: layout tests);
    inputs: gatk1_el / gatk1_er [U,H], gatc_el / gatc_er, gatb_gradout [N,H,D]."""
    from tests.golden import recipe
    to = lambda t: t.to(dev)  # noqa: E731
    rp, row, col = lists["sep_rel_ptrs"], lists["sep_row"], lists["sep_col"]
    E, n = row.numel(), gold["gatk1_sum"].shape[0]
    go = inputs["gatb_gradout"]
    H, D = go.shape[1], go.shape[2]
    ar = to(torch.arange(E))
    idx = (ar, to(rp), to(row), to(col))
    el, er = inputs["gatk1_el"], inputs["gatk1_er"]
    U = el.shape[0]
    gen = torch.Generator().manual_seed(77)
    featu, ret = torch.randn(U, H, D, generator=gen), torch.randn(n, H, D, generator=gen)
    # ---- kind 1 forward
    d1 = {"unique_srcs_and_dests_rel_ptrs": to(lists["ts_rel_ptrs"]), "unique_srcs_and_dests_node_indices": to(lists["ts_node_indices"])}
    sm, ex, rt = torch.full((n, H), 7.0, device=dev), torch.full((E, H), 7.0, device=dev), torch.full((n, H, D), 7.0, device=dev)
    ops.relational_fused_gat_separate_coo(*idx, 1, d1, to(featu), to(el), to(er), sm, ex, rt, slope)
    torch.testing.assert_close(cpu(ex), gold["gatk1_exp"], rtol=rtol_exp, atol=atol_exp)
    torch.testing.assert_close(cpu(sm), gold["gatk1_sum"], rtol=rtol_sum, atol=atol_sum)
    # ---- kind 2 forward: one inverse index (the row side of the two-sided list's) for both ends
    inv_row, _ = recipe.two_sided_inverse(lists["ts_inverse_indices"], rp)
    d2 = {"edata_idx_to_inverse_idx": to(inv_row)}
    sm2, ex2 = torch.full((n, H), 7.0, device=dev), torch.full((E, H), 7.0, device=dev)
    ops.relational_fused_gat_separate_coo(*idx, 2, d2, to(featu), to(el), to(er), sm2, ex2, rt, slope)
    torch.testing.assert_close(cpu(sm2), gold["gatk2_sum"], rtol=rtol_sum, atol=atol_sum)
    # ---- backward grad_feat, kinds 4 and 1, on the reference's own exp / sum
    d4 = {"edata_idx_to_inverse_idx_row": to(lists["ss_inverse_indices_row"]), "edata_idx_to_inverse_idx_col": to(lists["ss_inverse_indices_col"])}
    S_row = inputs["gatc_el"].shape[0]
    featc = torch.randn(S_row, H, D, generator=gen)
    cases = ((4, d4, featc, inputs["gatc_el"], inputs["gatc_er"], gold["gatc_sum"], gold["gatc_exp"], lists["ss_node_indices_row"],
              "gatcb_grad_feat_src"),
             (1, d1, featu, el, er, gold["gatk1_sum"], gold["gatk1_exp"], lists["ts_node_indices"], "gatk1b_grad_feat_src"))
    for kind, d, feat, l, r, s_ref, e_ref, node_of_row, key in cases:
        gf = torch.zeros(feat.shape[0], H, D, device=dev)
        gl, gr = torch.zeros(l.shape[0], H, device=dev), torch.zeros(r.shape[0], H, device=dev)
        ops.backward_relational_fused_gat_separate_coo(*idx, kind, d, to(feat), to(l), to(r), to(s_ref), to(e_ref), to(ret), to(go),
                                                       gf, gl, gr, slope)
        per_node = torch.zeros(n, H, D, dtype=torch.float64).index_add_(0, node_of_row, cpu(gf).double()).float()
        # fp32 sums of mixed-sign terms over a hub source's edges, in the reference's order on one side and in the kernels' (float
        # atomics when the groupings are off) on the other: the repository's fp32 tolerance, not the 5e-5 that
        # the kind-0 pin happens to meet -- 1 element of 589 104 on the full topology differs by 8.4e-5 relative with atomics
        torch.testing.assert_close(per_node, gold[key], rtol=2e-4, atol=2e-5)


# ---------------------------------------------------------------- inputs ON the leaky-ReLU kink, exact in every number format
TINY = 2.0 ** -30  # expf(TINY) rounds to 1.0f in fp32 (half an ulp of 1 is 2^-24)


def _grid(shape, values, gen):
    """A tensor of `shape` drawn uniformly from the list `values`."""
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def exact_rgat_case(g, H, K, D, seed, zero_rows=0.15, bias=True, self_loop=True):
    """Inputs of one RGAT layer on graph g drawn from small integer grids, so that every quantity a route forms on the way to the
    pre-activation z = el + er is exact in fp32 and in bf16, in any association: x in {-1, 0, 1} (a fraction `zero_rows` of the
    rows all zero: el = er = 0 there in every relation, so every edge between two such nodes sits exactly ON the leaky-ReLU
    kink), W in {-1, 0, 1} / 4 (feat = x . W: multiples of 1/4 up to K / 4, 7 significant bits at K = 64), attn_l / attn_r in
    {-1, 0, 1} / 2 (W . attn: multiples of 1/8; el, er, z: multiples of 1/8 below 2^11 / 8).  fp32, bf16 and fp64 therefore take the
    same branch at every (edge, head), and the derivative AT z == 0 is `slope` (oracle: z > 0 ? 1 : slope).  Returns a dict of
    fp32 CPU tensors: x [N,K], W [R,H,K,D], attn_l / attn_r [R,H,D], loop_weight [K,H*D] or None, h_bias [H*D] or None, go [N,H*D]
    (multiples of 1/4 in [-2, 2]: exact in bf16)."""
    gen = torch.Generator().manual_seed(seed)
    N, R = g.get_num_nodes(), g.get_num_rels()
    x = _grid((N, K), [-1.0, 0.0, 1.0], gen)
    x[torch.rand(N, generator=gen) < zero_rows] = 0.0
    return {"x": x,
            "W": _grid((R, H, K, D), [-0.25, 0.0, 0.25], gen),
            "attn_l": _grid((R, H, D), [-0.5, 0.0, 0.5], gen),
            "attn_r": _grid((R, H, D), [-0.5, 0.0, 0.5], gen),
            "loop_weight": _grid((K, H * D), [-0.25, 0.0, 0.25], gen) if self_loop else None,
            "h_bias": _grid((H * D,), [i / 8 for i in range(-8, 9)], gen) if bias else None,
            "go": _grid((N, H * D), [i / 4 for i in range(-8, 9)], gen)}


def rgat_case_preactivations(c, sep, dtype=torch.float64, folded=False, bf16_feat=False):
    """z [E,H] of an exact_rgat_case in `dtype`, as (x . W) . attn (literal) or x . (W . attn) (folded); bf16_feat: with the
    projected rows rounded to bf16 before the dot with attn (literal form only)."""
    R = c["W"].shape[0]
    rel = torch.repeat_interleave(torch.arange(R), sep["rel_ptrs"][1:] - sep["rel_ptrs"][:-1])
    x, W, al, ar = (c[n].to(dtype) for n in ("x", "W", "attn_l", "attn_r"))
    if folded:
        el_n = torch.einsum("nk,rhk->rnh", x, torch.einsum("rhkd,rhd->rhk", W, al))
        er_n = torch.einsum("nk,rhk->rnh", x, torch.einsum("rhkd,rhd->rhk", W, ar))
    else:
        feat = torch.einsum("nk,rhkd->rnhd", x, W)
        if bf16_feat:
            feat = feat.to(torch.bfloat16).to(dtype)
        el_n = (feat * al[:, None]).sum(-1)
        er_n = (feat * ar[:, None]).sum(-1)
    return el_n[rel, sep["row_indices"]] + er_n[rel, sep["col_indices"]]


def rgat_case_tie_stats(c, sep, num_nodes):
    """Where the ties of an exact_rgat_case sit: {"z": fp64 z [E,H], "tied_edges": edges with a tied head, "hub": tied edges ending
    at a destination of more than 256 in-edges, "deg1": ... of exactly one in-edge}."""
    z = rgat_case_preactivations(c, sep)
    tied = (z == 0).any(1)
    indeg = torch.bincount(sep["col_indices"], minlength=num_nodes)[sep["col_indices"]]
    return {"z": z, "tied_edges": int(tied.sum()), "hub": int((tied & (indeg > 256)).sum()), "deg1": int((tied & (indeg == 1)).sum())}


def assert_ties_on_hub_edges(c, sep, num_nodes, hub=1):
    """The property that makes a layer test a test AT the kink: its input has exact ties, `hub` of them on edges into destinations of
    more than 256 in-edges.  Asserted by every such test before it compares, so that a change of generator cannot quietly turn them
    back into off-kink tests."""
    st = rgat_case_tie_stats(c, sep, num_nodes)
    assert st["tied_edges"] > 0 and st["hub"] >= hub, f"no ties on hub edges: {st['tied_edges']} tied edges, {st['hub']} into hubs"
    return st


GAT_Z_CLASSES = ("tie", "tiny+", "tiny-", "ordinary")


def gat_z_class(z):
    """Class index (GAT_Z_CLASSES) of every pre-activation: 0 tie, 1 z = +2^-30, 2 z = -2^-30, 3 |z| >= 1/8; -1 anything else."""
    out = torch.full(z.shape, -1, dtype=torch.int64)
    out[z == 0] = 0
    out[z == TINY] = 1
    out[z == -TINY] = 2
    out[z.abs() >= 0.125] = 3
    return out


def exact_gat_case(srow, drow, col, ns, nd, num_nodes, H, D, seed, min_deg=8):
    """Op-level inputs at the kink for the fused-GAT pairs: feat [ns,H,D], el [ns,H], er [nd,H], go [num_nodes,H,D] for edges whose
    el / er rows are srow / drow (by position) and whose destinations are col.  Every z = el[srow] + er[drow] is an exact fp32 sum
    of one of four classes (GAT_Z_CLASSES): an exact tie z == 0; z = +2^-30 (expf rounds to 1.0f: the grouped kernels have to
    recover z > 0 from a stored exp that would be 1); z = -2^-30; an ordinary multiple of 1/8 with 1/8 <= |z| <= 4.  To keep the
    sums exact a row holding +-2^-30 only meets rows holding 0: the er rows of every destination of `min_deg` in-edges or more
    are 0 (its classes come from el: 0, +-2^-30, k/8), the other er rows are 0 or k/8, and an el row is +-2^-30 only where all
    its edges meet er == 0.  Every class occurs among the in-edges of every destination of `min_deg` or more in-edges, for every
    head: four of its source rows are pinned to the four classes (asserted).  feat in {-1, -1/2, 0, 1/2, 1}, go multiples of
    1/4 in [-2, 2] (both exact in bf16)."""
    gen = torch.Generator().manual_seed(seed)
    ordinary = [k / 8 for k in range(-16, 17) if k != 0]
    indeg = torch.bincount(col, minlength=num_nodes)
    big_edge = indeg[col] >= min_deg
    er = torch.where(torch.rand(nd, H, generator=gen) < 0.3, torch.zeros(nd, H), _grid((nd, H), ordinary, gen))
    er[drow[big_edge]] = 0.0
    meets_nonzero = torch.zeros(ns, H).index_add_(0, srow, (er[drow] != 0).float()) > 0  # [ns,H]
    u = torch.rand(ns, H, generator=gen)
    ordin = _grid((ns, H), ordinary, gen)
    el_free = torch.where(u < 0.3, torch.zeros(ns, H), torch.where(u < 0.55, torch.full((ns, H), TINY),
                          torch.where(u < 0.8, torch.full((ns, H), -TINY), ordin)))
    el = torch.where(meets_nonzero, torch.where(u < 0.15, torch.zeros(ns, H), ordin), el_free)
    # pin the four classes at every destination of min_deg or more in-edges (their er rows are 0: z = el there)
    pinned = torch.zeros(ns, H, dtype=torch.bool)
    order = torch.argsort(col, stable=True)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(indeg, 0)])
    want = (0.0, TINY, -TINY, 0.5)
    for v in torch.nonzero(indeg >= min_deg).flatten().tolist():
        rows = torch.unique(srow[order[ptr[v]:ptr[v + 1]]])
        for h in range(H):
            free = rows[~pinned[rows, h] & ~meets_nonzero[rows, h]][:4]
            assert free.numel() == 4, f"destination {v}, head {h}: fewer than four source rows that can take any class"
            el[free, h] = torch.tensor(want)
            pinned[free, h] = True
    feat = _grid((ns, H, D), [-1.0, -0.5, 0.0, 0.5, 1.0], gen)
    go = _grid((num_nodes, H, D), [i / 4 for i in range(-8, 9)], gen)
    return feat, el, er, go


def load_rgat_case(layer, c):
    """Copy the parameters of an exact_rgat_case into a HET_RGATLayer (same shapes; a parameter the case leaves out must be one the
    layer does not have); returns (x, go)."""
    have = dict(layer.named_parameters())
    with torch.no_grad():
        for name, key in (("conv_weights", "W"), ("attn_l", "attn_l"), ("attn_r", "attn_r"), ("loop_weight", "loop_weight"), ("h_bias", "h_bias")):
            assert (c[key] is not None) == (name in have), name
            if c[key] is not None:
                have[name].copy_(c[key].view(have[name].shape))
    return c["x"].clone(), c["go"].clone()


def gat_rows_of_kind(g, kind):
    """(srow, drow) by edge position: the rows of el / feat and of er that the fused-GAT pair of CompactAsOfNodeKind `kind` reads on
    graph g, and (ns, nd), the row counts."""
    from oracle import ops as O
    from tests.test_oracle import _gat_dict, _gat_sizes
    s = g.get_separate_coo_original()
    srow, drow = O._gat_rows(kind, _gat_dict(g, kind)[0], s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"])
    return srow, drow, _gat_sizes(g, kind)


def assert_gat_ties_on_hub_edges(el, er, srow, drow, col, num_nodes):
    """An op-level input has exact ties and the +-2^-30 classes on edges into destinations of more than 256 in-edges."""
    cls = gat_z_class(el.double()[srow] + er.double()[drow])
    hub = (torch.bincount(col, minlength=num_nodes) > 256)[col]
    for k in (0, 1, 2):
        assert int((cls[hub] == k).sum()) > 0, f"no z of class {GAT_Z_CLASSES[k]} on a hub edge"


def exact_gat_case_of_kind(g, kind, H, D, seed):
    """exact_gat_case for the rows of CompactAsOfNodeKind `kind` on graph g (ties on hub edges asserted)."""
    srow, drow, (ns, nd) = gat_rows_of_kind(g, kind)
    col, N = g.get_separate_coo_original()["col_indices"], g.get_num_nodes()
    feat, el, er, go = exact_gat_case(srow, drow, col, ns, nd, N, H, D, seed)
    assert_gat_ties_on_hub_edges(el, er, srow, drow, col, N)
    return feat, el, er, go
