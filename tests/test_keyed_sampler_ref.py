"""NeighborSampler(method="keyed") on CPU tensors: the sampling rule and the blocks against an independent numpy restatement
(tests/_keyed_sampler_ref.py), against method="sort" where no randomness is left, the block structure, the uniformity of the rule,
and HetGraph.from_block_separate_coo against from_integrated_coo.  No GPU; every test fails on a tree without the feature."""
import functools

import numpy as np
import pytest
import torch

from het_amd.graph import HetGraph
from het_amd.synth import IntegratedCOO, make_random
from tests import _keyed_sampler_ref as ref
from tests.util import ladder_graph

SEED = 5


@functools.lru_cache(maxsize=None)
def _graph(name, num_ntypes=1):
    if name == "random":
        return HetGraph.from_integrated_coo(make_random(400, 4, 6000, seed=13, num_ntypes=num_ntypes), full=True)
    assert num_ntypes == 1
    return ladder_graph()


def _seeds(g, name):
    if name == "random":
        return torch.tensor([5, 17, 99, 250, 3, 399, 0, 128])
    # ladder: a few rungs on both sides of the fan-outs (1, 3, 4, 5, 64), a hub, a split destination, an isolated node
    from tests.util import LADDER
    rung = {c: i for i, c in enumerate(LADDER)}
    return torch.tensor([rung[c] for c in (1, 3, 4, 5, 7, 63, 64, 65, 129, 513)] + [len(LADDER) + 1, g.get_num_nodes() - 1])


@pytest.mark.parametrize("by_type", [False, True])
@pytest.mark.parametrize("fanouts", [[3, 5], [1, 64], [-1, 4]])
@pytest.mark.parametrize("name", ["random", "ladder"])
def test_cpu_keyed_blocks_equal_the_numpy_reference(name, fanouts, by_type):
    """Field for field: nodes, num_dst, edge_ids, runs and every layout of graph_data, for two consecutive batches (draws 0, 1 and
    2, 3).  by_type runs on the random graph with three node types (the ladder has one type: its by_type case has one run per
    block and type)."""
    from het_amd.sampling import NeighborSampler
    g = _graph(name, 3 if (by_type and name == "random") else 1)
    csr = ref.Csr(g)
    s = NeighborSampler(g, fanouts, seed=SEED, by_type=by_type, method="keyed")
    seeds = _seeds(g, name)
    for batch in range(2):
        got = s.sample_blocks(seeds)
        want = ref.blocks(csr, seeds.numpy(), fanouts, SEED, by_type=by_type, first_draw=2 * batch)
        assert len(got) == len(want) == 2
        for l, (b, w) in enumerate(zip(got, want)):
            ref.assert_block_is_reference(b, w, g.get_num_rels(), True, f"{name} {fanouts} by_type={by_type} batch {batch} block {l}")


def test_keys_equal_the_reference_keys():
    """het_amd.sampling.keyed_keys (numpy uint64) against the plain-Python integers of the reference, also where the sums wrap and
    for negative / large seeds and draws."""
    from het_amd.sampling import keyed_keys
    pos = np.array([0, 1, 2, 63, 64, 1000, 123456, (1 << 32) + 5, (1 << 62) + 7], dtype=np.int64)
    for seed, draw in ((0, 0), (1, 0), (0, 1), (7, 12345), (-1, 3), ((1 << 64) - 1, (1 << 63) + 9)):
        want = np.array([ref.key_of(seed, draw, int(p)) for p in pos], dtype=np.uint64)
        got = keyed_keys(seed, draw, pos)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (seed, draw)
        assert np.array_equal(ref.keys_np(np.array([ref.stream_of(seed, draw)], dtype=np.uint64), pos)[0], want)


@pytest.mark.parametrize("by_type", [False, True])
@pytest.mark.parametrize("name", ["random", "ladder"])
def test_full_fanout_keyed_equals_sort(name, by_type):
    """Fan-out -1, and a fan-out at / above the largest in-degree: nothing is chosen, and "keyed" gives the blocks of "sort" in every
    field and layout."""
    from het_amd.sampling import NeighborSampler
    g = _graph(name, 3 if (by_type and name == "random") else 1)
    t = g.get_in_csr()
    max_deg = int((t["row_ptrs"][1:] - t["row_ptrs"][:-1]).max())
    seeds = _seeds(g, name)
    for fanouts in ([-1, -1], [max_deg, max_deg + 3], [-1, max_deg]):
        a = NeighborSampler(g, fanouts, seed=SEED, by_type=by_type, method="keyed").sample_blocks(seeds)
        b = NeighborSampler(g, fanouts, seed=SEED, by_type=by_type, method="sort").sample_blocks(seeds)
        for l, (x, y) in enumerate(zip(a, b)):
            ref.assert_same_block(x, y, f"{name} {fanouts} block {l}")


def test_keyed_blocks_structure_cpu():
    """The assertions of test_sampling.test_blocks_structure_cpu on keyed blocks; equal seeds agree, different seeds differ, and
    consecutive calls on one sampler differ (the draw counter advances)."""
    from het_amd.sampling import NeighborSampler
    coo = make_random(400, 4, 6000, seed=13)
    g = HetGraph.from_integrated_coo(coo, full=True)
    s = NeighborSampler(g, [3, 5], seed=1, method="keyed")
    seeds = torch.tensor([5, 17, 99, 250, 3])
    blocks = s.sample_blocks(seeds)
    assert len(blocks) == 2 and torch.equal(blocks[-1].nodes[: blocks[-1].num_dst], seeds)
    assert torch.equal(blocks[0].nodes[: blocks[0].num_dst], blocks[1].nodes)
    true_edges = set(zip(coo.row.tolist(), coo.col.tolist(), coo.rel.tolist()))
    for b, fan in zip(blocks, [3, 5]):
        sc = b.graph.get_separate_coo_original()
        assert torch.equal(sc["eids"], torch.arange(sc["eids"].numel()))
        src, dst = b.nodes[sc["row_indices"]], b.nodes[sc["col_indices"]]
        rel = torch.repeat_interleave(torch.arange(4), sc["rel_ptrs"][1:] - sc["rel_ptrs"][:-1])
        assert all((a, c, r) in true_edges for a, c, r in zip(src.tolist(), dst.tolist(), rel.tolist()))
        assert int(sc["col_indices"].max()) < b.num_dst
        indeg_block = torch.bincount(sc["col_indices"], minlength=b.num_dst)
        indeg_full = torch.bincount(coo.col, minlength=coo.num_nodes)[b.nodes[: b.num_dst]]
        assert torch.equal(indeg_block, torch.minimum(indeg_full, torch.tensor(fan)))
        assert torch.equal(coo.row[b.edge_ids], src) and torch.equal(coo.col[b.edge_ids], dst)
        extra = b.nodes[b.num_dst:]
        assert bool((extra[1:] > extra[:-1]).all())  # new nodes ascending by global id
    again = NeighborSampler(g, [3, 5], seed=1, method="keyed").sample_blocks(seeds)
    assert all(torch.equal(x.edge_ids, y.edge_ids) for x, y in zip(blocks, again))
    other = NeighborSampler(g, [3, 5], seed=2, method="keyed").sample_blocks(seeds)
    assert not all(torch.equal(x.edge_ids, y.edge_ids) for x, y in zip(blocks, other))
    nxt = s.sample_blocks(seeds)  # draws 2 and 3
    assert not torch.equal(blocks[-1].edge_ids, nxt[-1].edge_ids)
    # an explicit draw reproduces a block and leaves the counter alone
    one = s.sample_block(seeds, 5, draw=0)
    assert torch.equal(one.edge_ids, blocks[-1].edge_ids) and s._draw == 4
    with pytest.raises(ValueError):
        NeighborSampler(g, [3], method="hash")


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("deg,fanout,first", [(40, 5, 1000), (513, 20, 123456), (65, 64, 99), (9, 3, 5)])
def test_rule_is_uniform(seed, deg, fanout, first):
    """4000 draws of one destination: every edge's inclusion count within 5 standard deviations of draws * fanout / deg (a
    binomial count per edge).  Deterministic; with exactly this rule the worst of the twelve cases sits at 3.43."""
    from het_amd.sampling import keyed_keys
    draws = 4000
    pos = np.arange(first, first + deg, dtype=np.int64)
    streams = np.array([ref.stream_of(seed, d) for d in range(draws)], dtype=np.uint64)
    keys = ref.keys_np(streams, pos)
    for d in (0, 1, 3999):  # (the package's keys are these keys)
        assert np.array_equal(keyed_keys(seed, d, pos), keys[d])
    kept = np.argsort(keys, axis=1, kind="stable")[:, :fanout]  # the fanout smallest (key, pos) of every draw
    counts = np.bincount(kept.ravel(), minlength=deg)
    p = fanout / deg
    z = np.abs(counts - draws * p) / np.sqrt(draws * p * (1 - p))
    print(f"seed {seed} deg {deg} fanout {fanout}: worst deviation {z.max():.2f} sd")
    assert counts.sum() == draws * fanout and z.max() <= 5.0, z.max()


@pytest.mark.parametrize("full", [True, False])
def test_from_block_separate_coo_equals_from_integrated_coo(full):
    from het_amd.sampling import NeighborSampler
    g = _graph("random")
    b = NeighborSampler(g, [3, 5], seed=SEED, method="keyed", full_layouts=full).sample_blocks(torch.tensor([5, 17, 99, 250, 3]))[0]
    o, s = b.graph.graph_data["original"], b.graph.get_separate_coo_original()
    assert s["row_indices"].numel() > 0
    made = HetGraph.from_block_separate_coo(b.graph.get_num_nodes(), b.graph.get_num_rels(), o["node_type_offsets"], s["rel_ptrs"],
                                            s["row_indices"], s["col_indices"], o["rel_types"], full=full)
    coo = IntegratedCOO(b.graph.get_num_nodes(), b.graph.get_num_rels(), o["node_type_offsets"], o["row_indices"], o["col_indices"],
                        o["rel_types"], torch.arange(o["eids"].numel()))
    want = HetGraph.from_integrated_coo(coo, full=full)
    assert list(made.graph_data) == list(want.graph_data)
    ref.assert_same_graph_data(made.graph_data, want.graph_data)
    assert made.sequential_eids_format == want.sequential_eids_format == "separate_coo"
    assert made.get_num_nodes() == want.get_num_nodes() and made.get_num_rels() == want.get_num_rels()
    assert ("transposed" in made.graph_data) == full
    # the integrated and the separate COO share their tensors
    ms = made.graph_data["separate"]["coo"]["original"]
    assert ms["row_indices"] is made.graph_data["original"]["row_indices"] and ms["eids"] is made.graph_data["original"]["eids"]
    # an empty block
    z = torch.zeros(0, dtype=torch.int64)
    e = HetGraph.from_block_separate_coo(3, 2, torch.tensor([0, 3]), torch.zeros(3, dtype=torch.int64), z, z, z, full=full)
    w = HetGraph.from_integrated_coo(IntegratedCOO(3, 2, torch.tensor([0, 3]), z, z, z, z), full=full)
    ref.assert_same_graph_data(e.graph_data, w.graph_data)


def test_sampler_made_in_inference_mode_keeps_a_normal_map():
    from het_amd.sampling import NeighborSampler
    g = _graph("random")
    with torch.inference_mode():
        s = NeighborSampler(g, [3], seed=SEED, method="keyed")
    assert not s._map.is_inference()
    b = s.sample_blocks(torch.tensor([5, 17]))[0]  # (writes the map in place outside inference mode)
    assert bool((s._map == -1).all()) and b.num_dst == 2
