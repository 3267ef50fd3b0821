"""RGAT layer evaluation forward (torch.no_grad()) at the ogbn-mag shape, feat 64, 4 heads, with and without get_attention, on one box
and in one run.

    python exp/rgat_attention_ab.py [--steps 100] [--out profiles/r08/rgat_attention_ab.txt]

One child process per mode, interleaved (off, positions, destinations, torch, destinations, positions, off): a later process runs a
little faster on these boxes whatever it is, so a difference counts only if it shows in both orders.
  off           layer(g, x): no attention output
  positions     layer(g, x, get_attention=True), phase 2 in edge-position order (the default)
  destinations  the same with HET_RGAT_ATTN_ORDER=d: phase 2 walks the grouping by destination, scattered stores
  torch         layer(g, x) followed by rgat_fused_layer.attention_composition (what a call outside the evaluation paths gets)
Each child reports the call (HIP events around it, median) and, for the native modes, the two phases alone from the library's
per-kernel events (het_kernel_timing: phase 1 = HET_rgat_attn_lse with its finishing launch, phase 2 = HET_rgat_attn_rows) in a run
of their own."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("off", "positions", "destinations", "torch")


def child(mode, steps, heads, feat):
    import torch
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
    layer = HET_RGATLayer(feat, feat, R, heads, self_loop=True, dropout=0.0).to(dev).eval()
    x = torch.randn(N, feat, device=dev) * 0.3

    def call():
        if mode == "off":
            return layer(g, x), None
        if mode == "torch":
            h = layer(g, x)
            return h, FL.attention_composition(g, x, layer.conv_weights, layer.attn_l, layer.attn_r, layer.leaky_relu_slope)
        return layer(g, x, get_attention=True)

    with torch.no_grad():
        for _ in range(3):  # warm-up: unique lists, groupings, hub lists
            out, attn = call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        t = [s.elapsed_time(e) for s, e in ev]
        phases = {}
        if mode in ("positions", "destinations"):
            n = 20
            _lib.kernel_timing(True)
            for _ in range(n):
                call()
            torch.cuda.synchronize()
            phases = {"phase1_ms": _lib.kernel_timing_read("HET_rgat_attn_lse")[0] / n,
                      "phase2_ms": _lib.kernel_timing_read("HET_rgat_attn_rows")[0] / n}
            _lib.kernel_timing(False)
    q = statistics.quantiles(t, n=10)
    return {"mode": mode, "N": N, "E": E, "R": R, "device": torch.cuda.get_device_name(0), "library": _lib.build_info(),
            "median_ms": statistics.median(t), "mean_ms": statistics.mean(t), "p10_ms": q[0], "p90_ms": q[-1],
            "checksum": None if attn is None else float(attn.double().sum()), **phases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=MODES, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.heads, a.feat)))
        return
    res = []
    for mode in ("off", "positions", "destinations", "torch", "destinations", "positions", "off"):
        env = dict(os.environ)
        env.pop("HET_RGAT_ATTN_ORDER", None)
        if mode == "destinations":
            env["HET_RGAT_ATTN_ORDER"] = "d"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps if mode != "torch" else min(a.steps, 20)),
                            "--heads", str(a.heads), "--feat", str(a.feat)], capture_output=True, text=True, timeout=400, env=env)
        if r.returncode != 0:
            sys.exit(f"child {mode} failed ({r.returncode}): {r.stderr[-3000:]}")
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(res[-1], flush=True)
    r0 = res[0]
    E, H = r0["E"], a.heads
    model_p2 = E * (32 + 3 * 4 * H + 4 * H)  # ids, three 4H-byte row gathers, one 4H-byte row written
    model_p1 = E * (8 + 2 * 4 * H)           # two int32 payloads, an el and an er gather
    lines = [f"RGAT layer evaluation forward (torch.no_grad()) with / without get_attention, ogbn-mag shape (make_mag_like scale 1.0): "
             f"N={r0['N']} E={E} R={r0['R']}, feat {a.feat} -> {a.feat}, {H} heads, fp32, {r0['device']}", f"library: {r0['library']}",
             f"one process per line, in this order; {a.steps} calls each (torch: 20), HIP events around the call, ms; phases: the library's "
             "per-kernel events, ms per call, 20 calls",
             f"byte model: phase 1 {model_p1 / 1e6:.0f} MB requested, phase 2 {model_p2 / 1e6:.0f} MB requested (a scattered 4H-byte row "
             "moves a whole line)",
             f"  {'mode':13s} {'median':>9s} {'mean':>9s} {'p10':>9s} {'p90':>9s} {'phase 1':>9s} {'phase 2':>9s}  checksum"]
    for r in res:
        lines.append(f"  {r['mode']:13s} {r['median_ms']:9.4f} {r['mean_ms']:9.4f} {r['p10_ms']:9.4f} {r['p90_ms']:9.4f} "
                     f"{r.get('phase1_ms', float('nan')):9.4f} {r.get('phase2_ms', float('nan')):9.4f}  {r['checksum']}")
    med = {m: statistics.mean(r["median_ms"] for r in res if r["mode"] == m) for m in MODES}
    lines.append(f"  cost of the attention output (median over the call without it): positions {med['positions'] - med['off']:.4f} ms, "
                 f"destinations {med['destinations'] - med['off']:.4f} ms, torch composition {med['torch'] - med['off']:.4f} ms")
    for m in ("positions", "destinations"):
        p1 = statistics.mean(r["phase1_ms"] for r in res if r["mode"] == m)
        p2 = statistics.mean(r["phase2_ms"] for r in res if r["mode"] == m)
        lines.append(f"  {m}: phase 1 {p1:.4f} ms = {model_p1 / p1 / 1e9:.2f} TB/s of its model, phase 2 {p2:.4f} ms = "
                     f"{model_p2 / p2 / 1e9:.2f} TB/s of its model")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
