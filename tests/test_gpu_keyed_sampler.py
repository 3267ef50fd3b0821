"""NeighborSampler(method="keyed") on the GPU (csrc/block_sample.hip): the blocks equal, bit for bit, the blocks of the keyed CPU
path -- which tests/test_keyed_sampler_ref.py holds to an independent numpy restatement of the rule -- on the degree ladder, on rows
around every threshold of the selection kernels, over two layers with and without type-sorted runs, and on degenerate shapes; the
layers and the driver run on keyed blocks.

The selection is a most-significant-digit radix select, which is exact on its own: there is no candidate pass and therefore no
fallback to test.  The thresholds it exports (het_amd.kernels.sample_thresholds) are the in-degree from which a workgroup takes a
destination instead of a wave, and the positions per emission chunk of that workgroup."""
import functools

import numpy as np
import pytest
import torch

from het_amd.graph import HetGraph
from het_amd.synth import IntegratedCOO, make_mag_like
from tests import _keyed_sampler_ref as ref
from tests.util import LADDER, LADDER_SPLITS, ladder_graph

pytestmark = pytest.mark.gpu
SEED = 11


def _pair(make):
    """(CPU graph, the same graph on the GPU)."""
    return make(), make().to_("cuda")


@functools.lru_cache(maxsize=None)
def _ladder():
    return _pair(ladder_graph)


def _samplers(gc, gg, fanouts, **kw):
    from het_amd.sampling import NeighborSampler
    return (NeighborSampler(gc, fanouts, seed=SEED, method="keyed", **kw), NeighborSampler(gg, fanouts, seed=SEED, method="keyed", **kw))


@pytest.mark.parametrize("fanout", [1, 4, 63, 64, 65, 256, 512, -1])
def test_ladder_blocks_equal_the_cpu_blocks(fanout):
    """Every rung destination (in-degrees 1 .. 769), every split destination and three isolated nodes as seeds: deg < fanout,
    deg == fanout, deg == fanout + 1 and deg >> fanout on both sides of the wave width and of the workgroup threshold."""
    gc, gg = _ladder()
    n_dst = len(LADDER) + len(LADDER_SPLITS)
    N = gc.get_num_nodes()
    seeds = torch.cat([torch.arange(n_dst), torch.tensor([N - 1, N - 4, N - 7])])
    sc, sg = _samplers(gc, gg, [fanout])
    for draw in (0, 5):
        want = sc.sample_block(seeds, fanout, draw=draw)
        got = sg.sample_block(seeds.cuda(), fanout, draw=draw)
        assert got.nodes.is_cuda and got.graph.get_device().type == "cuda"
        ref.assert_same_block(got, want, f"ladder fanout {fanout} draw {draw}")
        assert bool((sg._map == -1).all())
    if fanout == 4:  # the sample is the rule's: the reference module's own choice for one rung
        csr = ref.Csr(gc)
        w = ref.block(csr, seeds.numpy(), fanout, SEED, 5)
        assert torch.equal(got.edge_ids.cpu(), torch.from_numpy(w["edge_ids"])) and torch.equal(got.nodes.cpu(), torch.from_numpy(w["nodes"]))


def _threshold_degrees():
    import het_amd.kernels as k
    t = k.sample_thresholds()
    T = sorted({t["workgroup_degree"], t["chunk"]})
    return T, [d for x in T for d in (x - 1, x, x + 1)] + [20001]


@functools.lru_cache(maxsize=None)
def _long_rows():
    """Destinations of in-degree T - 1, T, T + 1 for every exported threshold T, and one of 20 001, behind 1000 filler nodes whose
    edges come first in the in-CSR; 3 relations."""
    _, degs = _threshold_degrees()

    def make():
        gen = torch.Generator().manual_seed(3)
        pool = 1000
        N = pool + len(degs)
        fill = 4000
        row = [torch.randint(0, pool, (fill,), generator=gen)] + [torch.randint(0, pool, (d,), generator=gen) for d in degs]
        col = [torch.randint(0, pool, (fill,), generator=gen)] + [torch.full((d,), pool + i) for i, d in enumerate(degs)]
        row, col = torch.cat(row), torch.cat(col)
        rel = torch.randint(0, 3, (row.numel(),), generator=gen)
        o = torch.sort(rel, stable=True).indices
        return HetGraph.from_integrated_coo(IntegratedCOO(N, 3, torch.tensor([0, N]), row[o], col[o], rel[o], torch.arange(row.numel())))
    return _pair(make)


def test_long_row_blocks_equal_the_cpu_blocks():
    """Whole blocks on the long-row graph, fan-outs 1, 25 and every threshold T.  The rows start at the largest positions this graph
    gives (about 4000 .. 30 000); positions above 2^32 are covered by test_selection_above_2_to_32 below, on the selection entry
    alone, since a graph of more than 2^32 edges is not practical in a test."""
    T, degs = _threshold_degrees()
    gc, gg = _long_rows()
    N = gc.get_num_nodes()
    seeds = torch.cat([torch.arange(N - len(degs), N), torch.tensor([3, 500])])
    ptr = gc.get_in_csr()["row_ptrs"]
    assert sorted((ptr[seeds + 1] - ptr[seeds])[: len(degs)].tolist()) == sorted(degs)
    for fanout in [1, 25] + T:
        sc, sg = _samplers(gc, gg, [fanout])
        ref.assert_same_block(sg.sample_block(seeds.cuda(), fanout, draw=2), sc.sample_block(seeds, fanout, draw=2), f"long rows fanout {fanout}")


def test_selection_above_2_to_32():
    """het_sample_count + het_sample_select read the row pointers only, so rows whose first position lies above 2^32 need no edge
    arrays: the long-row degrees, every row starting above 2^32, fan-outs 1, 25 and every threshold T, against the rule evaluated in
    numpy (het_amd.sampling.keyed_keys, held to the reference's integers by the CPU tests)."""
    import het_amd.kernels as k
    from het_amd.sampling import keyed_keys
    T, degs = _threshold_degrees()
    degs = degs + [0, 1, 63, 64, 65]
    base = (1 << 32) + 12345
    ptr = torch.tensor([base] + degs).cumsum(0)
    dst = torch.tensor([5, 0, 3, 1, 2, 4] + list(range(6, len(degs))))  # not in row order
    for fanout in [1, 25] + T:
        offsets, total = k.sample_count(ptr.cuda(), dst.cuda(), fanout)
        kept = [min(degs[v], fanout) for v in dst.tolist()]
        assert total == sum(kept) and offsets.cpu().tolist() == [0] + np.cumsum(kept).tolist()
        pos, owner = k.sample_select(ptr.cuda(), dst.cuda(), fanout, SEED, 9, offsets, total)
        want_pos, want_owner = [], []
        for b, v in enumerate(dst.tolist()):
            p = np.arange(int(ptr[v]), int(ptr[v + 1]), dtype=np.int64)
            if len(p) > fanout:
                p = np.sort(p[np.argsort(keyed_keys(SEED, 9, p), kind="stable")[:fanout]])
            want_pos.append(p)
            want_owner.append(np.full(len(p), b, dtype=np.int64))
        assert int(pos.min()) > (1 << 32)
        assert torch.equal(pos.cpu(), torch.from_numpy(np.concatenate(want_pos))), f"fanout {fanout}: pos"
        assert torch.equal(owner.cpu(), torch.from_numpy(np.concatenate(want_owner))), f"fanout {fanout}: owner"


@functools.lru_cache(maxsize=None)
def _mag():
    return _pair(lambda: HetGraph.from_integrated_coo(make_mag_like(scale=4e-4), full=True))


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("by_type", [False, True])
def test_two_layers_equal_the_cpu_blocks(by_type, full):
    gc, gg = _mag()
    N = gc.get_num_nodes()
    seeds = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:40]
    sc, sg = _samplers(gc, gg, [4, 6], by_type=by_type, full_layouts=full)
    for batch in range(2):  # (the draw counters advance in step: draws 0, 1 and 2, 3)
        want, got = sc.sample_blocks(seeds), sg.sample_blocks(seeds.cuda())
        for l, (x, y) in enumerate(zip(got, want)):
            ref.assert_same_block(x, y, f"mag by_type={by_type} batch {batch} block {l}")
        assert bool((sg._map == -1).all()), "the scratch map is all -1 after a call"
    assert got[0].graph.get_num_edges() > 0 and got[0].nodes.numel() > got[0].num_dst
    # the same draw again: the same bits
    _, sg2 = _samplers(gc, gg, [4, 6], by_type=by_type, full_layouts=full)
    sg2._draw = 2
    for x, y in zip(sg2.sample_blocks(seeds.cuda()), got):
        ref.assert_same_block(x, y, "second call with the same draws")
    b = got[-1]
    dst, T = b.nodes[: b.num_dst], gc.get_num_ntypes()
    dst_runs = (b.runs[0][:T], b.runs[1][: T + 1]) if by_type else None  # (the runs of the seeds: the first T of the block's)
    one, two = sg.sample_block(dst, 6, dst_runs, draw=2), sg.sample_block(dst, 6, dst_runs, draw=2)
    ref.assert_same_block(one, two, "sample_block twice with draw=2")
    assert torch.equal(one.edge_ids, b.edge_ids)


def test_sampler_made_in_inference_mode_serves_evaluation():
    gc, gg = _mag()
    from het_amd.sampling import NeighborSampler
    seeds = torch.arange(0, gc.get_num_nodes(), 37)[:16].cuda()
    with torch.inference_mode():
        s = NeighborSampler(gg, [4], seed=SEED, method="keyed")
        inside = s.sample_block(seeds, 4, draw=0)
    assert not s._map.is_inference()
    outside = s.sample_block(seeds, 4, draw=0)
    ref.assert_same_block(inside, outside, "inference mode")
    assert not outside.graph.holds_inference_tensors()


@pytest.mark.parametrize("one_shot", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_rgat_on_keyed_blocks_matches_the_oracle_on_the_blocks(compact, one_shot):
    """The body of test_sampling.test_rgat_on_sampled_blocks_matches_the_oracle_on_the_blocks with method="keyed"."""
    import contextlib
    from het_amd.layers import HET_RGATLayer
    from het_amd.sampling import NeighborSampler, one_shot_graphs, run_blocks
    from tests.test_sampling import _graph, _oracle_rgat_on_blocks
    from tests.util import assert_close
    coo, g = _graph("cuda")
    torch.manual_seed(6)
    flags = dict(compact_as_of_node_flag=compact, compact_direct_indexing_flag=compact, self_loop=True, dropout=0.0)
    layers = torch.nn.ModuleList([HET_RGATLayer(64, 64, 4, 4, activation=torch.relu, **flags),
                                  HET_RGATLayer(64, 64, 4, 1, **flags)]).cuda()
    x = torch.randn(coo.num_nodes, 64, device="cuda", requires_grad=True)
    seeds = torch.tensor([7, 300, 42, 9, 111, 250, 18, 77], device="cuda")
    blocks = NeighborSampler(g, [4, 6], seed=3, method="keyed").sample_blocks(seeds)
    indeg = torch.bincount(coo.col, minlength=coo.num_nodes)
    assert int(indeg[blocks[-1].nodes[: blocks[-1].num_dst]].max()) > 6  # the fan-out really truncates neighbourhoods
    go = torch.randn(seeds.numel(), 64, device="cuda")
    with (one_shot_graphs(blocks) if one_shot else contextlib.nullcontext()):
        out = run_blocks(layers, blocks, x[blocks[0].nodes])
        out.backward(go)
    x64 = x.detach().double().cpu()[blocks[0].nodes.cpu()].requires_grad_(True)
    want, params = _oracle_rgat_on_blocks(layers, blocks, x64)
    want.backward(go.double().cpu())
    assert_close(out, want, what="out")
    gx = torch.zeros(coo.num_nodes, 64, dtype=torch.float64).index_add_(0, blocks[0].nodes.cpu(), x64.grad)
    assert_close(x.grad, gx, what="grad_x")
    for layer, p in zip(layers, params):
        for name in ("conv_weights", "attn_l", "attn_r", "loop_weight", "h_bias"):
            assert_close(getattr(layer, name).grad, p[name].grad, what="grad_" + name)


def test_rgcn_on_full_fanout_keyed_blocks_and_driver():
    from het_amd import train
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    from het_amd.sampling import NeighborSampler, run_blocks
    from tests.test_sampling import _graph
    coo, g = _graph("cuda")
    torch.manual_seed(4)
    layer = HET_EglRelGraphConv_EdgeParallel(64, 64, 4).cuda()
    x, norm = torch.randn(coo.num_nodes, 64, device="cuda"), torch.rand(coo.num_edges, 1, device="cuda")
    full = layer(g, x, norm)
    seeds = torch.tensor([1, 2, 3, 399], device="cuda")
    b = NeighborSampler(g, [-1], method="keyed").sample_blocks(seeds)
    out = run_blocks([layer], b, x[b[0].nodes], norm)
    torch.testing.assert_close(out, full[seeds], rtol=2e-4, atol=2e-5)
    res = train.main(["--model", "rgat", "-d", "mag", "--scale", "0.01", "--n_infeat", "64", "--num_classes", "64",
                      "--num_heads", "4", "--num_layers", "2", "--fanout", "5", "10", "--batch_size", "256",
                      "--n_epochs", "6", "--dropout", "0.0", "--keyed_sampler"])
    assert res["sampler"] == "keyed" and res["args"]["keyed_sampler"] is True
    assert res["minibatch_sample_and_layout_ms"] is not None and res["final_loss"] < 4.3


def test_degenerate_shapes():
    """Empty seeds, seeds that are all isolated, a fan-out above every degree: well-formed blocks, equal to the CPU path's."""
    gc, gg = _ladder()
    N = gc.get_num_nodes()
    n_dst = len(LADDER) + len(LADDER_SPLITS)
    for full in (True, False):
        for seeds, fanout, edges in ((torch.zeros(0, dtype=torch.int64), 4, 0), (torch.tensor([N - 1, N - 2, N - 5]), 4, 0),
                                     (torch.tensor([N - 3]), -1, 0), (torch.arange(n_dst), 100000, None)):
            sc, sg = _samplers(gc, gg, [fanout], full_layouts=full)
            got, want = sg.sample_block(seeds.cuda(), fanout), sc.sample_block(seeds, fanout)
            ref.assert_same_block(got, want, f"degenerate {seeds.numel()} seeds fanout {fanout} full={full}")
            if edges == 0:
                assert torch.equal(got.nodes.cpu(), seeds) and got.graph.get_num_edges() == 0
            else:
                ptr = gc.get_in_csr()["row_ptrs"]
                assert got.graph.get_num_edges() == int((ptr[seeds + 1] - ptr[seeds]).sum())
            assert bool((sg._map == -1).all())
    torch.cuda.synchronize()
