"""The RGCN layer with block-diagonal relation weights (regularizer="bdd"): the native route against the dense expansion, and the
basis layer with dense W_r for scale -- one layer, forward and backward timed separately, on one box in one process.

    python exp/rgcn_bdd_ab.py [--steps 200] [--shapes wikikg2 aifb mag] [--out profiles/r18/rgcn_bdd_ab.txt]

Variants (interleaved in rounds of 10 steps, HIP events around the forward and around the backward):
  native  the bdd layer on csrc/rgcn_bdd.hip                        (layer.last_route == "native", asserted)
  dense   the same layer with HET_RGCN_BDD=0: the blocks expanded to [R, K, D], the layer's existing code
  basis   HET_EglRelGraphConv_EdgeParallel(K, D, R) with dense W_r at the same R, K, D
Shapes: the wikikg2-sized random graph of exp/many_relations.py (N = 2 500 604, E = 16 109 182, R = 535), the AIFB-sized graph at
104 relations, the ogbn-mag shape at R = 4; 64 -> 64, B = 8.  Then the library's per-kernel times over 50 native steps with the
byte model of the two new passes (node pass: S * 4K + N * 4D; weight gradient: S * 4 (K + D)), and the peak memory of one step of
each variant above what was allocated before it.  (The kernel timers match by prefix: the line HET_rgcn_bdd_dw, and the rate
computed from it, include the finish launch listed below it.)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from het_amd import _lib  # noqa: E402
from het_amd.graph import HetGraph  # noqa: E402
from het_amd.layers import HET_EglRelGraphConv_EdgeParallel  # noqa: E402
from het_amd.synth import make_aifb_like, make_mag_like, make_random  # noqa: E402

KERNELS = ("HET_segment_sum", "HET_rgcn_bdd_node_pass", "HET_rgcn_bdd_dw", "HET_rgcn_bdd_dw_finish", "HET_colsum")
SHAPES = {"wikikg2": lambda: make_random(2500604, 535, 16109182, seed=1), "aifb": lambda: make_aifb_like(num_rels=104),
          "mag": lambda: make_mag_like(scale=1.0)}
K = D = 64
B = 8


def run(name, steps, lines):
    dev = "cuda"
    coo = SHAPES[name]()
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    g = HetGraph.from_integrated_coo(coo, full=True)
    N, E, R = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels()
    torch.manual_seed(0)
    bdd = HET_EglRelGraphConv_EdgeParallel(K, D, R, B, regularizer="bdd").to(dev)
    basis = HET_EglRelGraphConv_EdgeParallel(K, D, R).to(dev)
    norm, x, go = torch.rand(E, 1, device=dev), torch.randn(N, K, device=dev), torch.randn(N, D, device=dev)
    variants = {"native": (bdd, "native"), "dense": (bdd, "0"), "basis": (basis, "1")}  # (native: also where the route prefers dense)

    def step(v, ev=None):
        layer, switch = variants[v]
        os.environ["HET_RGCN_BDD"] = switch
        layer.zero_grad(set_to_none=True)
        xd = x.detach().requires_grad_(True)
        if ev:
            ev[0].record()
        out = layer(g, xd, norm)
        if ev:
            ev[1].record()
        out.backward(go)
        if ev:
            ev[2].record()
        if layer is bdd:
            assert layer.last_route == v, (v, layer.last_route)

    lines.append(f"--- {name}: N={N} E={E} R={R}, {K} -> {D}, B={B}")
    for v in list(variants) * 2:  # warm-up: groupings, row lists, maps, the sorted norm
        step(v)
    torch.cuda.synchronize()
    times = {v: ([], []) for v in variants}
    for _ in range((steps + 9) // 10):
        for v in variants:
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(10)]
            for ev in evs:
                step(v, ev)
            torch.cuda.synchronize()
            times[v][0].extend(a.elapsed_time(b) for a, b, _ in evs)
            times[v][1].extend(b.elapsed_time(c) for _, b, c in evs)
    lines.append(f"  {'variant':8s} {'fwd median':>11s} {'fwd p10':>9s} {'fwd p90':>9s} {'bwd median':>11s} {'bwd p10':>9s} {'bwd p90':>9s}   (ms, "
                 f"{len(times['native'][0])} steps each)")
    for v, (f, b) in times.items():
        qf, qb = statistics.quantiles(f, n=10), statistics.quantiles(b, n=10)
        lines.append(f"  {v:8s} {statistics.median(f):11.4f} {qf[0]:9.4f} {qf[-1]:9.4f} {statistics.median(b):11.4f} {qb[0]:9.4f} {qb[-1]:9.4f}")
    med = {v: statistics.median(f) + statistics.median(b) for v, (f, b) in times.items()}
    lines.append(f"  native / dense (fwd + bwd medians): {med['native'] / med['dense']:.3f}   native / basis: {med['native'] / med['basis']:.3f}")

    from het_amd import kernels as k
    s = g.get_separate_coo_original()
    S_dst = k._plan.get_grouping(s["rel_ptrs"], s["col_indices"], N, s["row_indices"], s["eids"]).num_segments
    S_src = k._plan.get_grouping(s["rel_ptrs"], s["row_indices"], N, s["col_indices"], s["eids"]).num_segments
    _lib.kernel_timing(True)
    for _ in range(50):
        step("native")
    torch.cuda.synchronize()
    per = {kn: _lib.kernel_timing_read(kn) for kn in KERNELS}
    _lib.kernel_timing(False)
    lines.append(f"  per-kernel time of the native step, 50 steps (ms per step; launches per step); rows: S_dst={S_dst} S_src={S_src}")
    for kn, (ms, n) in per.items():
        lines.append(f"    {kn:24s} {ms / 50:8.4f} {n / 50:4.0f}")
    node_bytes = (S_dst * 4 * K + N * 4 * D) + (S_src * 4 * D + N * 4 * K)  # the forward's and the backward's node pass
    dw_bytes = S_dst * 4 * (K + D)
    for kn, nbytes in (("HET_rgcn_bdd_node_pass", node_bytes), ("HET_rgcn_bdd_dw", dw_bytes)):
        ms = per[kn][0] / 50
        if ms > 0:
            lines.append(f"    {kn}: {nbytes / 1e9:.3f} GB by the byte model -> {nbytes / ms / 1e9:.2f} TB/s")
    lines.append("  peak memory of one step above what was allocated before it (MiB):")
    for v in variants:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(v)
        torch.cuda.synchronize()
        lines.append(f"    {v:8s} {(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f}")
    os.environ.pop("HET_RGCN_BDD", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"RGCN bdd layer, native against dense expansion against the basis layer, {torch.cuda.get_device_name(0)}",
             f"library: {_lib.build_info()}"]
    for name in a.shapes:
        run(name, a.steps, lines)
        print("\n".join(lines), flush=True)
        if a.out:  # (rewritten after every shape: a later shape that runs out of time or memory loses nothing)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
