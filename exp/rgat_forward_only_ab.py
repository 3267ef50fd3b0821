"""RGAT layer forward under torch.no_grad() at the ogbn-mag shape, feat 64, 4 heads: the training forward (what a no_grad call ran
before the forward-only path: HET_RGAT_FORWARD_ONLY=0) against the forward-only path, on one box.

    python exp/rgat_forward_only_ab.py [--steps 200] [--out profiles/r07/rgat_forward_only_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python exp/rgat_forward_only_ab.py --only forward_only --steps 20

Without --only: four child processes, one mode each, in both orders (training, forward_only, forward_only, training) -- the second
process of a pair runs 0.2-0.5 % faster on these boxes whatever it is, so a difference counts only if it shows in both orders.  The
training instances' device code is byte-identical to the parent commit's (exp/tools/isa_diff.py), so mode `training` on this
library IS the parent's forward.  Each child reports the layer forward (HIP events around layer(g, x), median), the three aggregate
launches (het_kernel_timing: the library's own events, serialising -- a run of its own) and the peak memory of one call."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("HET_rgat_aggregate_packs", "HET_rgat_aggregate_hubs", "HET_rgat_aggregate_finish")


def child(mode, steps):
    os.environ["HET_RGAT_FORWARD_ONLY"] = "1" if mode == "forward_only" else "0"
    import torch
    from het_amd import _lib
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import make_mag_like
    dev = "cuda"
    coo = make_mag_like(scale=1.0)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    g = HetGraph.from_integrated_coo(coo, full=True)
    N, E, R = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels()
    torch.manual_seed(0)
    layer = HET_RGATLayer(64, 64, R, 4, self_loop=True, dropout=0.0).to(dev).eval()
    x = torch.randn(N, 64, device=dev) * 0.3
    with torch.no_grad():
        for _ in range(5):  # warm-up: unique lists, groupings, hub lists
            out = layer(g, x)
        torch.cuda.synchronize()
        if steps < 0:  # (--only: steps for a profiler, nothing else)
            for _ in range(-steps):
                layer(g, x)
            torch.cuda.synchronize()
            return None
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for s, e in ev:
            s.record()
            layer(g, x)
            e.record()
        torch.cuda.synchronize()
        t = [s.elapsed_time(e) for s, e in ev]
        _lib.kernel_timing(True)
        for _ in range(50):
            layer(g, x)
        torch.cuda.synchronize()
        per = {k: _lib.kernel_timing_read(k)[0] / 50 for k in KERNELS}
        _lib.kernel_timing(False)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        layer(g, x)
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    q = statistics.quantiles(t, n=10)
    return {"mode": mode, "N": N, "E": E, "R": R, "device": torch.cuda.get_device_name(0), "library": _lib.build_info(),
            "median_ms": statistics.median(t), "mean_ms": statistics.mean(t), "p10_ms": q[0], "p90_ms": q[-1], "kernels_ms": per,
            "peak_MiB": peak, "checksum": float(out.double().sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("training", "forward_only"), default=None, help="warm up, run --steps calls of this mode, nothing else")
    ap.add_argument("--child", choices=("training", "forward_only"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.only:
        child(a.only, -a.steps)
        print(f"{a.steps} calls of {a.only} done")
        return
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps)))
        return
    res = []
    for mode in ("training", "forward_only", "forward_only", "training"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps)], capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"child {mode} failed ({r.returncode}): {r.stderr[-3000:]}")
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    r0 = res[0]
    lines = [f"RGAT layer forward under torch.no_grad(), ogbn-mag shape (make_mag_like scale 1.0): N={r0['N']} E={r0['E']} R={r0['R']}, "
             f"feat 64 -> 64, 4 heads, {r0['device']}", f"library: {r0['library']}",
             f"one process per line, in this order; {a.steps} calls each (HIP events around the layer, ms); kernels: het_kernel_timing, "
             "ms per call, 50 calls, serialised",
             f"  {'mode':13s} {'median':>8s} {'mean':>8s} {'p10':>8s} {'p90':>8s} {'packs':>8s} {'hubs':>8s} {'finish':>8s} {'peak MiB':>9s}"]
    for r in res:
        k = r["kernels_ms"]
        lines.append(f"  {r['mode']:13s} {r['median_ms']:8.4f} {r['mean_ms']:8.4f} {r['p10_ms']:8.4f} {r['p90_ms']:8.4f} "
                     f"{k[KERNELS[0]]:8.4f} {k[KERNELS[1]]:8.4f} {k[KERNELS[2]]:8.4f} {r['peak_MiB']:9.1f}")
    lines.append(f"  forward_only / training (median): first pair {res[1]['median_ms'] / res[0]['median_ms']:.3f}, "
                 f"second pair {res[2]['median_ms'] / res[3]['median_ms']:.3f}")
    lines.append("  output checksums equal: " + str(len({r["checksum"] for r in res}) == 1))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
