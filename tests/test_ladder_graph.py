"""The threshold-ladder graph of tests/util.py (CPU only): every prescribed count is present, measured with bincount on the graph's
own layouts, so that the GPU tests of tests/test_gpu_thresholds.py land exactly on the thresholds they are written for."""
import pytest
import torch

from tests.util import (LADDER, LADDER_SPLITS, ROW_LADDER, assert_ladder, assert_rungs, ladder_counts, ladder_graph,
                        row_ladder_ptrs)


@pytest.mark.parametrize("seed", [0, 1])
def test_ladder_graph_has_every_rung(seed):
    g = ladder_graph(R=5, seed=seed)
    assert_ladder(g)
    c = ladder_counts(g)
    # the thresholds themselves and their neighbours, spelled out
    for t in (32, 64, 256):
        assert_rungs(c["in_rel"], (t - 1, t, t + 1), f"in-degree per (relation, destination) around {t}")
        assert_rungs(c["out_rel"], (t - 1, t, t + 1), f"out-degree per (relation, source) around {t}")
    assert g.get_num_edges() < 20000  # (the fp64 oracle stays quick)
    # eids are a permutation, not arange
    s = g.get_separate_coo_original()
    assert not torch.equal(s["eids"], torch.arange(g.get_num_edges()))
    assert torch.equal(torch.sort(s["eids"]).values, torch.arange(g.get_num_edges()))


def test_ladder_graph_split_destinations():
    """The destinations whose in-edges span relations: totals of 256 / 257 (and 32 / 33, 64 / 65) made of runs that are each
    shorter, and hubs with a run longer than one work item."""
    g = ladder_graph(R=5)
    s = g.get_separate_coo_original()
    N, R = g.get_num_nodes(), g.get_num_rels()
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    runs = torch.bincount(rel * N + s["col_indices"], minlength=R * N).view(R, N)
    tot = runs.sum(0)
    for total, parts in LADDER_SPLITS:
        hit = [v for v in range(N) if int(tot[v]) == total and sorted(runs[:, v][runs[:, v] > 0].tolist()) == sorted(parts)]
        assert hit, (total, parts)
    multi = (runs > 0).sum(0)
    assert bool(((tot == 256) & (multi >= 2) & (runs.max(0).values < 256)).any())
    assert bool(((tot == 257) & (multi >= 2) & (runs.max(0).values < 256)).any())
    assert bool(((tot > 256) & (runs.max(0).values > 256) & (multi >= 2)).any())


@pytest.mark.parametrize("R", [1, 7, 8, 9, 12])
def test_ladder_graph_relation_counts(R):
    """The relation-count ladder of the layer tests: R relations (one empty from R = 4 on), single-relation rungs still exact."""
    g = ladder_graph(R=R, shuffle=False)
    assert g.get_num_rels() == R
    c = ladder_counts(g)
    assert_rungs(c["in_rel"], LADDER, "in-degree per (relation, destination)")
    assert_rungs(c["out_rel"], LADDER, "out-degree per (relation, source)")
    assert int((c["rel"] == 0).sum()) == (1 if R >= 4 else 0)


def test_row_ladder():
    rp = row_ladder_ptrs()
    counts = (rp[1:] - rp[:-1]).tolist()
    assert sorted(counts) == sorted((0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097)) and tuple(counts) == ROW_LADDER
    # relation boundaries inside 32-row tiles
    assert sum(int(b) % 32 != 0 for b in rp[1:-1]) >= 6
