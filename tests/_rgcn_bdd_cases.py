"""The graphs and shapes of the bdd layer's tests (tests/test_gpu_rgcn_bdd.py runs them on the GPU, tests/test_rgcn_bdd_ref.py
checks on the CPU that their integer-grid inputs are exact in fp32 in any summation order).  No GPU import here."""
import functools

import torch

from het_amd.graph import HetGraph
from het_amd.synth import IntegratedCOO, make_random
from tests.util import ROW_LADDER, ladder_graph, permute_eids

SHAPES = ((32, 32, 8), (64, 64, 8), (64, 64, 4), (64, 64, 16), (64, 32, 2), (32, 64, 4), (128, 128, 4))  # (K, D, B)
REL_COUNTS = (0, 1, 2, 3, 4, 7, 8, 9, 10, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
REL_COUNT_R = 200


def _graph(N, R, row, col, rel, seed):
    o = torch.sort(rel, stable=True).indices
    coo = IntegratedCOO(N, R, torch.tensor([0, N]), row[o], col[o], rel[o], torch.arange(row.numel(), dtype=torch.int64))
    g = HetGraph.from_integrated_coo(coo)
    permute_eids(g, seed + 1000)
    return g


def rel_count_graph(seed=3, pool=300):
    """R = 200; destination i and source len(REL_COUNTS) + i have edges in exactly REL_COUNTS[i] relations (one or two edges in each),
    the other ends taken from a pool of nodes that are never rungs.  Neighbouring node ids get different counts."""
    gen = torch.Generator().manual_seed(seed)
    n = len(REL_COUNTS)
    pool0, N = 2 * n, 2 * n + pool + 5
    rows, cols, rels = [], [], []
    for i, c in enumerate(REL_COUNTS):
        for side in (0, 1):
            rr = torch.randperm(REL_COUNT_R, generator=gen)[:c]
            rr = torch.cat([rr, rr[: c // 2]])  # (half of the relations get a second edge)
            other = pool0 + torch.randint(0, pool, (rr.numel(),), generator=gen)
            rung = torch.full((rr.numel(),), i if side == 0 else n + i)
            rows.append(other if side == 0 else rung)
            cols.append(rung if side == 0 else other)
            rels.append(rr)
    return _graph(N, REL_COUNT_R, torch.cat(rows), torch.cat(cols), torch.cat(rels), seed)


def rel_counts_of(g):
    """(relations per destination, relations per source) as measured on a graph."""
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    per = lambda idx: torch.bincount(torch.unique(rel * N + idx) % N, minlength=N)  # noqa: E731
    return per(s["col_indices"]), per(s["row_indices"])


def row_ladder_counts(chunk):
    return ROW_LADDER + (chunk - 1, chunk, chunk + 1, 2 * chunk + 5)


def row_ladder_graph(chunk, seed=4):
    """Relation r has row_ladder_counts(chunk)[r] distinct destinations (0 included; chunk - 1, chunk, chunk + 1 rows and one relation
    of several chunks), one to three in-edges each."""
    gen = torch.Generator().manual_seed(seed)
    counts = row_ladder_counts(chunk)
    N = max(counts) + 37
    rows, cols, rels = [], [], []
    for r, c in enumerate(counts):
        dst = torch.randperm(N, generator=gen)[:c]
        dst = torch.cat([dst, dst[: c // 2], dst[: c // 4]])
        rows.append(torch.randint(0, N, (dst.numel(),), generator=gen))
        cols.append(dst)
        rels.append(torch.full((dst.numel(),), r, dtype=torch.int64))
    return _graph(N, len(counts), torch.cat(rows), torch.cat(cols), torch.cat(rels), seed)


def rows_per_relation(g):
    """Distinct destinations per relation."""
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    return torch.bincount(torch.unique(rel * N + s["col_indices"]) // N, minlength=R)


def many_rel_graph(R, n=211, e=2500, seed=5):
    """A random graph of R relations (every one of them non-empty when e >> R)."""
    g = HetGraph.from_integrated_coo(make_random(n, R, e, seed=seed))
    permute_eids(g, seed + 1000)
    return g


def repeat_graph(seed=6):
    """For the same-bits test: 12 relations of about 5 000 edges each on 6 000 nodes -- relations that span several chunks, several
    relations per node, a few edges per (relation, node) pair (the test asserts at most 32)."""
    g = HetGraph.from_integrated_coo(make_random(6000, 12, 60000, seed=seed))
    permute_eids(g, seed + 1000)
    return g


@functools.lru_cache(maxsize=None)
def graph(name, arg=0):
    """The CPU graph of a name: "ladder" (ladder_graph(R=5)), "relcount", "rowladder" (arg = chunk rows), "rels" (arg = R), "repeat"."""
    if name == "ladder":
        return ladder_graph(R=5)
    if name == "relcount":
        return rel_count_graph()
    if name == "rowladder":
        return row_ladder_graph(arg)
    if name == "rels":
        return many_rel_graph(arg)
    if name == "repeat":
        return repeat_graph()
    raise KeyError(name)


def coo_of(g):
    """(src, dst, rel, eid) by position of a graph's separate COO."""
    s = g.get_separate_coo_original()
    rel = torch.repeat_interleave(torch.arange(g.get_num_rels()), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    return s["row_indices"], s["col_indices"], rel, s["eids"]
