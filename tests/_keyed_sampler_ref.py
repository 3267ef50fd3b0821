"""An independent restatement, in numpy and plain Python, of the keyed sampling rule and of the block a NeighborSampler builds from
it (het_amd/sampling.py's docstring).  It shares no code with het_amd.sampling and never imports it: the tests hold
the package's CPU path to this, and the HIP path to the CPU path.

    sm(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
    stream = sm(seed ^ sm(draw))        key(pos) = sm(stream + pos)             (uint64, wrapping)
"""
import numpy as np

M = (1 << 64) - 1


def sm(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def stream_of(seed, draw):
    return sm((seed & M) ^ sm(draw & M))


def key_of(seed, draw, pos):
    return sm((stream_of(seed, draw) + pos) & M)


def keys_np(streams, pos):
    """key of every (stream, pos) pair: streams [S] and pos [P] as uint64 arrays -> [S, P] uint64."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = streams.astype(u)[:, None] + pos.astype(u)[None, :]
        z = z + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))


def kept_positions(start, deg, fanout, seed, draw):
    """The in-CSR positions one destination keeps, ascending."""
    every = list(range(start, start + deg))
    if fanout <= 0 or deg <= fanout:
        return every
    return sorted(sorted(every, key=lambda p: (key_of(seed, draw, p), p))[:fanout])


class Csr:
    """The in-CSR of a graph as numpy arrays (rows = destinations)."""

    def __init__(self, g):
        t = g.get_in_csr()
        self.ptr, self.src, self.rel, self.eid = (t[k].cpu().numpy() for k in ("row_ptrs", "col_indices", "rel_types", "eids"))
        self.num_nodes, self.num_rels = g.get_num_nodes(), g.get_num_rels()
        self.type_offsets = g.get_original_node_type_offsets().cpu().numpy()

    def type_of(self, nodes):
        T = len(self.type_offsets) - 1
        return np.minimum(np.searchsorted(self.type_offsets[1:], nodes, side="right"), T - 1)


def block(csr, dst, fanout, seed, draw, dst_runs=None):
    """One block as a dict of numpy arrays: nodes, num_dst, edge_ids, row / col / rel (block edges, relation-major, local ids),
    node_offs (the block's node_type_offsets) and runs ((types, offsets) or None)."""
    dst = np.asarray(dst, dtype=np.int64)
    B = len(dst)
    pos, owner = [], []
    for b, v in enumerate(dst.tolist()):
        kept = kept_positions(int(csr.ptr[v]), int(csr.ptr[v + 1] - csr.ptr[v]), fanout, seed, draw)
        pos += kept
        owner += [b] * len(kept)
    pos, owner = np.asarray(pos, dtype=np.int64), np.asarray(owner, dtype=np.int64)
    src = csr.src[pos]
    is_dst = set(dst.tolist())
    extra = np.asarray(sorted(set(src.tolist()) - is_dst), dtype=np.int64)
    nodes = np.concatenate([dst, extra])
    local = {int(v): i for i, v in enumerate(nodes.tolist())}
    assert len(local) == len(nodes), "destinations are distinct"
    o = np.argsort(csr.rel[pos], kind="stable")
    out = {"nodes": nodes, "num_dst": B, "edge_ids": csr.eid[pos][o],
           "row": np.asarray([local[int(s)] for s in src[o]], dtype=np.int64), "col": owner[o], "rel": csr.rel[pos][o]}
    T = len(csr.type_offsets) - 1
    if dst_runs is None:
        out["runs"], out["node_offs"] = None, np.asarray([0, len(nodes)], dtype=np.int64)
    else:
        counts = np.bincount(csr.type_of(extra), minlength=T) if len(extra) else np.zeros(T, dtype=np.int64)
        types = np.concatenate([dst_runs[0], np.arange(T)])
        offs = np.concatenate([dst_runs[1], B + np.cumsum(counts)])
        out["runs"], out["node_offs"] = (types, offs), offs
    return out


def blocks(csr, seeds, fanouts, seed, by_type=False, first_draw=0):
    """The blocks of one sample_blocks call, first layer first; the last layer's block is drawn first (draw = first_draw), as the
    sampler walks from the seeds outwards."""
    dst, runs = np.asarray(seeds, dtype=np.int64), None
    if by_type:
        T = len(csr.type_offsets) - 1
        t = csr.type_of(dst)
        dst = dst[np.argsort(t, kind="stable")]
        runs = (np.arange(T), np.concatenate([[0], np.cumsum(np.bincount(t, minlength=T))]))
    out, draw = [], first_draw
    for fanout in reversed(list(fanouts)):
        b = block(csr, dst, fanout, seed, draw, runs)
        draw += 1
        out.insert(0, b)
        dst, runs = b["nodes"], b["runs"]
    return out


# ---- comparison helpers of the tests (torch side) ----------------------------------------------------------------------------
def assert_same_graph_data(a, b, path="graph_data"):
    """Two graph_data dicts: the same keys in the same nesting, equal tensors (device aside)."""
    import torch
    assert isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b), f"{path}: keys {sorted(a)} != {sorted(b)}"
    for k in a:
        if isinstance(a[k], dict):
            assert_same_graph_data(a[k], b[k], f"{path}[{k!r}]")
        else:
            x, y = a[k].cpu(), b[k].cpu()
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f"{path}[{k!r}] differs"


def assert_same_block(x, y, what=""):
    """Two het_amd.sampling.Block objects, field for field: nodes, num_dst, edge_ids, runs, every tensor of graph.graph_data."""
    import torch
    eq = lambda s, t: s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.cpu(), t.cpu())  # noqa: E731
    assert x.num_dst == y.num_dst, f"{what}: num_dst"
    assert eq(x.nodes, y.nodes), f"{what}: nodes"
    assert eq(x.edge_ids, y.edge_ids), f"{what}: edge_ids"
    assert (x.runs is None) == (y.runs is None), f"{what}: runs"
    if x.runs is not None:
        assert eq(x.runs[0], y.runs[0]) and eq(x.runs[1], y.runs[1]), f"{what}: runs"
    assert x.graph.get_num_nodes() == y.graph.get_num_nodes() and x.graph.get_num_rels() == y.graph.get_num_rels(), f"{what}: sizes"
    assert x.graph.sequential_eids_format == y.graph.sequential_eids_format == "separate_coo"
    assert_same_graph_data(x.graph.graph_data, y.graph.graph_data, f"{what}: graph_data")


def assert_block_is_reference(b, ref, num_rels, full, what=""):
    """A Block of the package against a reference block (the dict `block` returns): the reference's edges go through
    HetGraph.from_integrated_coo, the builder the rest of the suite pins, and every layout is compared."""
    import torch
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))  # noqa: E731
    assert b.num_dst == ref["num_dst"], f"{what}: num_dst"
    assert torch.equal(b.nodes.cpu(), t(ref["nodes"])), f"{what}: nodes"
    assert torch.equal(b.edge_ids.cpu(), t(ref["edge_ids"])), f"{what}: edge_ids"
    assert (b.runs is None) == (ref["runs"] is None), f"{what}: runs"
    coo = IntegratedCOO(len(ref["nodes"]), num_rels, t(ref["node_offs"]), t(ref["row"]), t(ref["col"]), t(ref["rel"]),
                        torch.arange(len(ref["row"]), dtype=torch.int64))
    want = HetGraph.from_integrated_coo(coo, full=full)
    if ref["runs"] is not None:
        assert torch.equal(b.runs[0].cpu(), t(ref["runs"][0])) and torch.equal(b.runs[1].cpu(), t(ref["runs"][1])), f"{what}: runs"
        want.graph_data["original"]["node_segment_types"] = t(ref["runs"][0])
    assert_same_graph_data(b.graph.graph_data, want.graph_data, f"{what}: graph_data")
