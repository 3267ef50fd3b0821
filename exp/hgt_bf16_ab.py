"""fp32 vs bf16 activations for one HGT layer step (forward + backward) at the ogbn-mag shape, feat 64, 8 heads (BASELINE.json
configs[3]), on one box.

    python exp/hgt_bf16_ab.py [--steps 200] [--out profiles/r06/hgt_bf16_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python exp/hgt_bf16_ab.py --only bf16 --steps 20   (one dtype's steps alone)

The two dtypes run interleaved in rounds of 10 steps (same graph and layer; the bf16 step gets the bf16-rounded h and
gradout), each step timed with HIP events; then per-kernel times (het_kernel_timing: the library's own events) over 50 steps of
each, and the peak memory of one step of each (torch.cuda.max_memory_allocated after a reset, above what was allocated before)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from het_amd import _lib  # noqa: E402
from het_amd.graph import HetGraph  # noqa: E402
from het_amd.layers import HET_HGTLayerHetero  # noqa: E402
from het_amd.synth import make_mag_like  # noqa: E402

KERNELS = ("HET_hgt_aggregate_rows", "HET_hgt_backward_dst_rows", "HET_hgt_backward_src_short", "HET_hgt_backward_src_long",
           "HET_seg_gemm_mfma", "HET_seg_dw_mfma", "HET_node_rows_sum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fp32", "bf16"), default=None, help="warm up, run --steps steps of this dtype, nothing else")
    a = ap.parse_args()
    dev = "cuda"
    coo = make_mag_like(scale=1.0)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    g = HetGraph.from_integrated_coo(coo, full=True)
    N, E, R, T = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels(), g.get_num_ntypes()
    torch.manual_seed(0)
    layer = HET_HGTLayerHetero(T, R, 64, 64, num_heads=8, dropout=0.0).to(dev)
    x32, go32 = torch.randn(N, 64, device=dev) * 0.5, torch.randn(N, 64, device=dev)
    inputs = {"fp32": (x32, go32), "bf16": (x32.to(torch.bfloat16), go32.to(torch.bfloat16))}

    def step(dt):
        x, go = inputs[dt]
        layer.zero_grad(set_to_none=True)
        xd = x.detach().requires_grad_(True)
        out = layer(g, xd)
        out.backward(go)

    lines = [f"HGT layer fwd+bwd, ogbn-mag shape (make_mag_like scale 1.0): N={N} E={E} R={R} T={T}, feat 64 -> 64, 8 heads, "
             f"{torch.cuda.get_device_name(0)}", f"library: {_lib.build_info()}"]
    for dt in ("fp32", "bf16", "fp32", "bf16"):  # warm-up: groupings, lists, plans
        step(dt)
    torch.cuda.synchronize()
    if a.only:
        for _ in range(a.steps):
            step(a.only)
        torch.cuda.synchronize()
        print(f"{a.steps} steps of {a.only} done")
        return
    times = {"fp32": [], "bf16": []}
    rounds = (a.steps + 9) // 10
    for _ in range(rounds):
        for dt in ("fp32", "bf16"):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
            for s, e in ev:
                s.record()
                step(dt)
                e.record()
            torch.cuda.synchronize()
            times[dt] += [s.elapsed_time(e) for s, e in ev]
    lines.append(f"step time, {rounds * 10} steps each, interleaved in rounds of 10 (HIP events, ms):")
    lines.append(f"  {'dtype':6s} {'median':>8s} {'mean':>8s} {'p10':>8s} {'p90':>8s}")
    for dt, t in times.items():
        q = statistics.quantiles(t, n=10)
        lines.append(f"  {dt:6s} {statistics.median(t):8.4f} {statistics.mean(t):8.4f} {q[0]:8.4f} {q[-1]:8.4f}")
    lines.append(f"  bf16 / fp32 (median): {statistics.median(times['bf16']) / statistics.median(times['fp32']):.3f}")

    lines.append("per-kernel time per step, 50 steps each (het_kernel_timing, ms per step; launches per step):")
    lines.append(f"  {'kernel':28s} {'fp32':>8s} {'bf16':>8s} {'ratio':>7s} {'launches':>9s}")
    per = {}
    for dt in ("fp32", "bf16"):
        _lib.kernel_timing(True)
        for _ in range(50):
            step(dt)
        torch.cuda.synchronize()
        per[dt] = {k: _lib.kernel_timing_read(k) for k in KERNELS}
        _lib.kernel_timing(False)
    for k in KERNELS:
        (m32, n32), (m16, n16) = per["fp32"][k], per["bf16"][k]
        ratio = f"{m16 / m32:7.3f}" if m32 > 0 else "      -"
        lines.append(f"  {k:28s} {m32 / 50:8.4f} {m16 / 50:8.4f} {ratio} {n32 / 50:4.0f}/{n16 / 50:<4.0f}")

    lines.append("peak memory of one step above what was allocated before it (MiB):")
    for dt in ("fp32", "bf16"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(dt)
        torch.cuda.synchronize()
        lines.append(f"  {dt:6s} {(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f}")
    x_mib = {dt: inputs[dt][0].numel() * inputs[dt][0].element_size() / 2**20 for dt in inputs}
    lines.append(f"  (the input h itself, allocated before the step: fp32 {x_mib['fp32']:.1f}, bf16 {x_mib['bf16']:.1f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
