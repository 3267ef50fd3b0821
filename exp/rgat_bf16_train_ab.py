"""RGAT layer training step (forward + backward) at the ogbn-mag shape, feat 64, 4 heads and 2 heads: fp32 input against bf16 input on
a layer built with bf16_training=True (the native bf16 step), on one box and in one run.

    python exp/rgat_bf16_train_ab.py [--steps 100] [--heads 4 2] [--out profiles/r09/rgat_bf16_train_ab.txt]

Per head count four child processes, one mode each, in both orders (fp32, bf16, bf16, fp32): the second process of a pair runs a
little faster on these boxes whatever it is, so a difference counts only if it shows in both orders.  Each child is a fresh process
with a time limit of its own.  It reports the step (HIP events around layer(g, x) and out.backward(go), median), the peak memory of
one step, and the time of each entry point of the step from events around the C calls (het_amd.kernels.event_timers) in a run of
its own with the side stream off, so that no two of them overlap."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# what the table calls each C entry of the two steps
PARTS = {"het_rgnn_relational_matmul_attn_dot": "project", "het_rows_matmul_heads_bf16": "project",
         "het_rgnn_relational_matmul": "er", "het_rows_dot1h_bf16": "er",
         "het_rows_linear_bias": "loop", "het_rows_linear_bias_bf16": "loop",
         "het_rgat_el_rows_bf16": "el",
         "het_rgat_aggregate_compact_runs": "aggregate", "het_rgat_aggregate_compact_runs_bf16": "aggregate",
         "het_rgat_backward_compact_runs": "edge_bwd", "het_rgat_backward_compact_runs_bf16": "edge_bwd",
         "het_rgat_node_backward_dx": "node_dx", "het_rgat_node_backward_dx_bf16": "node_dx",
         "het_rows_matmul_backward_dw": "dW", "het_rows_matmul_backward_dw_bf16": "dW",
         "het_rows_matmul_backward_dw_colsum": "dW_loop", "het_rows_matmul_backward_dw_bf16_bf16": "dW_loop",
         "het_backward_rgnn_relational_matmul": "dwa", "het_rows_dot1h_backward_dw_bf16": "dwa"}
COLS = ("project", "er", "loop", "el", "aggregate", "edge_bwd", "node_dx", "dW", "dW_loop", "dwa")


def child(mode, steps, heads, feat):
    import torch
    import het_amd.kernels as k
    from het_amd import _lib
    from het_amd.backend import rgat_fused_layer as FL
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
    layer = HET_RGATLayer(feat, feat, R, heads, self_loop=True, dropout=0.0, bf16_training=True).to(dev)
    x = (torch.randn(N, feat, device=dev) * 0.3).to(torch.bfloat16)  # the same values in both modes
    go = torch.randn(N, feat, device=dev).to(torch.bfloat16)
    if mode == "fp32":
        x, go = x.float(), go.float()
    x.requires_grad_(True)

    def step():
        x.grad = None
        layer.zero_grad(set_to_none=True)
        out = layer(g, x)
        out.backward(go)
        return out

    native = {"n": 0}
    agg = k.rgat_aggregate_compact_bf16
    k.rgat_aggregate_compact_bf16 = lambda *a, **kw: (native.__setitem__("n", native["n"] + 1), agg(*a, **kw))[1]
    for _ in range(5):  # warm-up: unique lists, groupings, hub lists, node maps
        out = step()
    torch.cuda.synchronize()
    assert out.dtype == x.dtype and x.grad.dtype == x.dtype and (native["n"] == 5) == (mode == "bf16")
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for s, e in ev:
        s.record()
        step()
        e.record()
    torch.cuda.synchronize()
    t = [s.elapsed_time(e) for s, e in ev]
    x.grad = None
    layer.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    FL.OVERLAP = False  # per entry point, nothing beside it
    rec = k.event_timers["*"] = []
    n_part = 30
    for _ in range(n_part):
        step()
    torch.cuda.synchronize()
    del k.event_timers["*"]
    per = dict.fromkeys(COLS, 0.0)
    for a, b, cname in rec:
        if cname in PARTS:
            per[PARTS[cname]] += a.elapsed_time(b) / n_part
    q = statistics.quantiles(t, n=10)
    return {"mode": mode, "heads": heads, "N": N, "E": E, "R": R, "device": torch.cuda.get_device_name(0), "library": _lib.build_info(),
            "median_ms": statistics.median(t), "mean_ms": statistics.mean(t), "p10_ms": q[0], "p90_ms": q[-1], "parts_ms": per,
            "peak_MiB": peak, "checksum": float(out.double().sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--heads", type=int, nargs="+", default=[4, 2])
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child_timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", choices=("fp32", "bf16"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.heads[0], a.feat)))
        return
    lines = []
    for heads in a.heads:
        res = []
        for mode in ("fp32", "bf16", "bf16", "fp32"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps), "--heads", str(heads),
                                "--feat", str(a.feat)], capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:  # (nothing more is started on the GPU after a child that failed)
                sys.exit(f"child {mode} ({heads} heads) failed ({r.returncode}): {r.stderr[-3000:]}")
            res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        r0 = res[0]
        lines += [f"RGAT layer training step (forward + backward), ogbn-mag shape (make_mag_like scale 1.0): N={r0['N']} E={r0['E']} R={r0['R']}, "
                  f"feat {a.feat} -> {a.feat}, {heads} heads, {r0['device']}", f"library: {r0['library']}",
                  f"one process per line, in this order; {a.steps} steps each (HIP events around the step, ms); parts: events around the C "
                  "entry points, ms per step, 30 steps, side stream off",
                  f"  {'mode':5s} {'median':>8s} {'mean':>8s} {'p10':>8s} {'p90':>8s} " + " ".join(f"{c:>9s}" for c in COLS) + f" {'peak MiB':>9s}"]
        for r in res:
            lines.append(f"  {r['mode']:5s} {r['median_ms']:8.4f} {r['mean_ms']:8.4f} {r['p10_ms']:8.4f} {r['p90_ms']:8.4f} "
                         + " ".join(f"{r['parts_ms'][c]:9.4f}" for c in COLS) + f" {r['peak_MiB']:9.1f}")
        lines.append(f"  bf16 / fp32 (median step): first pair {res[1]['median_ms'] / res[0]['median_ms']:.3f}, "
                     f"second pair {res[2]['median_ms'] / res[3]['median_ms']:.3f}")
        for c in COLS:
            f32 = (res[0]["parts_ms"][c] + res[3]["parts_ms"][c]) / 2
            b16 = (res[1]["parts_ms"][c] + res[2]["parts_ms"][c]) / 2
            if f32 > 0:
                lines.append(f"  {c}: bf16 / fp32 {b16 / f32:.3f} ({f32:.4f} -> {b16:.4f} ms)")
            elif b16 > 0:
                lines.append(f"  {c}: bf16 only {b16:.4f} ms")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
