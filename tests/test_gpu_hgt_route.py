"""The link between the record of hgt_route.decide and the launches of the HGT layer: for every case, the route the layer computed,
one forward + backward, and the calls of the kernels.py functions that tell the routes apart, counted and held against what the
record says.  Values are checked against the fp64 oracle by test_gpu_layers.py, test_gpu_hgt_bf16.py and test_gpu_hgt_use_norm.py;
the records themselves, on the CPU, by test_hgt_route.py."""
import collections
import functools

import pytest
import torch

from tests.util import mag_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTED = ("hgt_aggregate_compact", "hgt_aggregate_compact_bf16", "node_rows_matmul_sum", "node_rows_matmul_sum_bf16",
           "rows_matmul_backward_dx", "matmul_backward", "rows_matmul_bf16")


@functools.lru_cache(maxsize=None)
def _graph(name):
    """``mag``: the ogbn-mag-like graph; ``relsK``: K relations leaving node type 1 (test_gpu_layers.py:
    test_hgt_layer_fused_node_major_input_gradient_launches), 4 of them more than the node-major pass keeps in LDS."""
    from het_amd.graph import HetGraph
    from het_amd.synth import make_hetero_graph
    if name == "mag":
        return mag_graph(1.5e-3)
    rels = [(0, 2, 900)] + [(1, 1 + (i % 2), 700 + 50 * i) for i in range(int(name[4:]))]
    return HetGraph.from_integrated_coo(make_hetero_graph([150, 200, 120], rels, seed=5))


# graph, heads, in, out, the input gradient of the attention node in fp32, whether a bf16 input runs on the bf16 kernels
CASES = [("rels1", 4, 64, 64, "node_major", True), ("rels3", 4, 64, 64, "node_major", True), ("rels4", 4, 64, 64, "per_relation", True),
         ("mag", 4, 64, 64, "node_major", True), ("mag", 8, 64, 256, "per_relation", False), ("mag", 4, 128, 128, "per_relation", False),
         ("mag", 2, 64, 10, "per_relation", False)]


@pytest.mark.parametrize("compact_dst", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("graph,H,in_dim,out_dim,dx,native", CASES)
def test_the_record_is_what_runs(graph, H, in_dim, out_dim, dx, native, bf16, compact_dst, monkeypatch):
    import het_amd.kernels as k
    from het_amd.backend import hgt_fused_layer
    from het_amd.layers import HET_HGTLayerHetero
    monkeypatch.setattr(hgt_fused_layer, "COMPACT_DST_BELOW", 2.0 if compact_dst else 0.0)
    g = _graph(graph)
    torch.manual_seed(4)
    N = g.get_num_nodes()
    layer = HET_HGTLayerHetero(g.get_num_ntypes(), g.get_num_rels(), in_dim, out_dim, num_heads=H, dropout=0.0).to(DEV)
    routes, calls = [], collections.Counter()
    decide = layer._route
    monkeypatch.setattr(layer, "_route", lambda *a: (routes.append(decide(*a)), routes[-1])[1])
    for name in COUNTED:
        monkeypatch.setattr(k, name, lambda *a, _name=name, _real=getattr(k, name), **kw: (calls.update([_name]), _real(*a, **kw))[1])
    dtype = torch.bfloat16 if bf16 else torch.float32
    h = (torch.randn(N, in_dim) * 0.5).to(DEV, dtype).requires_grad_(True)
    g.to_(DEV)
    try:
        out = layer(g, h)
        out.backward(torch.randn(N, out_dim).to(DEV, dtype))
        torch.cuda.synchronize()
    finally:
        g.cpu_()
    assert out.dtype == dtype and h.grad.dtype == dtype and bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(h.grad.float()).all())
    # the record: a bf16 input outside the bf16 kernels is upcast, and the fp32 call routed again
    assert [r.path for r in routes] == (["upcast", "fused"] if bf16 and not native else ["fused"]), routes
    r = routes[-1]
    assert r.native_bf16 == (bf16 and native) and r.compact_dst == compact_dst, r
    assert r.dx == (dx if not r.native_bf16 or dx == "node_major" else "fp32_buffer"), r
    # the launches
    G = r.groups
    per_relation = r.dx == "per_relation"
    want = {
        "hgt_aggregate_compact": 0 if r.native_bf16 else G,
        "hgt_aggregate_compact_bf16": 1 if r.native_bf16 else 0,
        "rows_matmul_bf16": 4 if r.native_bf16 else 0,  # q, kv_c, the output projection and its input gradient
        "rows_matmul_backward_dx": G * (2 if r.dx == "fp32_buffer" else (int(r.compact_dst and r.split_q) + int(r.split_kv)) if per_relation else 0)
                                   + int(r.out_proj == "rows_scatter"),
        "matmul_backward": G * (int(r.compact_dst and not r.split_q) + int(not r.split_kv)) if per_relation else 0,
    }
    assert {name: calls[name] for name in want} == want, (r, calls)
    node_sum, other = "node_rows_matmul_sum", "node_rows_matmul_sum_bf16"
    if r.native_bf16:
        node_sum, other = other, node_sum
    assert calls[other] == 0 and (1 <= calls[node_sum] <= G * g.get_num_ntypes() if r.dx == "node_major" else calls[node_sum] == 0), (r, calls)
    assert r.out_proj == ("bf16_rows" if r.native_bf16 else "typed_gemm" if not compact_dst else
                          "rows_scatter" if k.rows_matmul_backward_split_ok(1, out_dim, out_dim) else "gemm_index_copy"), r
