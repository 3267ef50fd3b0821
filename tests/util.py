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
