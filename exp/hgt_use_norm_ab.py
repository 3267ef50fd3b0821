"""HGT layer step (forward + backward) with and without use_norm at the ogbn-mag shape, feat 64, 8 heads, on one box, and the typed
LayerNorm kernel pair alone against the torch composition of the same function.

    python exp/hgt_use_norm_ab.py [--steps 100] [--out profiles/r10/hgt_use_norm_ab.txt]

One process per mode, in the order off, on, on, off (a process reports the median / p10 / p90 of its steps, HIP events, and the
peak memory of one step above what was allocated before it); then one process that times, for fp32 and bf16 rows at X = 64 and
X = 256 on the graph's node-type runs, the kernel pair (het_kernel_timing: the library's own events around each launch; GB/s
from 2 N X sizeof(T) forward, 3 N X sizeof(T) backward) and, with HIP events around the whole call, the pair through autograd
against F.layer_norm per type slice + cat with its autograd backward."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _graph():
    import torch
    from het_amd.graph import HetGraph
    from het_amd.synth import make_mag_like
    coo = make_mag_like(scale=1.0)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to("cuda"))
    return HetGraph.from_integrated_coo(coo, full=True), torch


def _timed(fn, steps):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    t = [s.elapsed_time(e) for s, e in ev]
    q = statistics.quantiles(t, n=10)
    return statistics.median(t), q[0], q[-1]


def layer_mode(use_norm, steps):
    g, torch = _graph()
    from het_amd.layers import HET_HGTLayerHetero
    N = g.get_num_nodes()
    torch.manual_seed(0)
    layer = HET_HGTLayerHetero(g.get_num_ntypes(), g.get_num_rels(), 64, 64, num_heads=8, dropout=0.0, use_norm=use_norm).to("cuda")
    x, go = torch.randn(N, 64, device="cuda") * 0.5, torch.randn(N, 64, device="cuda")

    def step():
        layer.zero_grad(set_to_none=True)
        xd = x.detach().requires_grad_(True)
        layer(g, xd).backward(go)

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    med, p10, p90 = _timed(step, steps)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
    print(f"RESULT use_norm={'on ' if use_norm else 'off'} step median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}  ({steps} steps)  "
          f"peak memory of a step {peak:.1f} MiB  [N={N} E={g.get_num_edges()} {torch.cuda.get_device_name(0)}]")


def kernel_pair(steps):
    g, torch = _graph()
    import torch.nn.functional as F
    from het_amd import _lib
    from het_amd.backend.hgt_fused_layer import typed_layer_norm
    offs = g.get_original_node_type_offsets()
    bounds = offs.tolist()
    N, T = bounds[-1], len(bounds) - 1
    print(f"RESULT kernel pair alone, N={N} rows in {T} runs {bounds}; library: {_lib.build_info()}")
    print(f"RESULT {'rows':5s} {'X':>4s} {'fwd ms':>8s} {'GB/s':>7s} {'bwd ms':>8s} {'GB/s':>7s} {'colsum ms':>9s} | {'HIP f+b ms':>10s} {'torch f+b ms':>12s} {'torch/HIP':>9s}")
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for X in (64, 256):
            torch.manual_seed(1)
            y = (torch.randn(N, X, device="cuda") * 2 + 1).to(dtype).requires_grad_(True)
            go = torch.randn(N, X, device="cuda").to(dtype)
            gamma = (torch.rand(T, X, device="cuda") + 0.5).requires_grad_(True)
            beta = (torch.rand(T, X, device="cuda") * 2 - 1).requires_grad_(True)

            def hip():
                y.grad = gamma.grad = beta.grad = None
                typed_layer_norm(y, offs, gamma, beta, 1e-5).backward(go)

            def composed():
                y.grad = gamma.grad = beta.grad = None
                parts = [F.layer_norm(y[a:b], (X,), gamma[t].to(dtype), beta[t].to(dtype), 1e-5)
                         for t, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
                torch.cat(parts).backward(go)

            for fn in (hip, composed, hip, composed):
                fn()
            torch.cuda.synchronize()
            t_hip, t_torch = _timed(hip, steps)[0], _timed(composed, steps)[0]
            _lib.kernel_timing(True)
            for _ in range(steps):
                hip()
            torch.cuda.synchronize()
            (a_ms, a_n), (b_ms, b_n), (c_ms, c_n) = (_lib.kernel_timing_read(k) for k in  # (a prefix match: the first reads all three)
                                                     ("HET_rows_layer_norm", "HET_rows_layer_norm_backward", "HET_rows_layer_norm_colsum"))
            f_ms, f_n = a_ms - b_ms - c_ms, a_n - b_n - c_n
            _lib.kernel_timing(False)
            f_ms, b_ms, c_ms = f_ms / max(1, f_n), b_ms / max(1, b_n), c_ms / max(1, b_n)
            nbytes = N * X * y.element_size()
            print(f"RESULT {name:5s} {X:4d} {f_ms:8.4f} {2 * nbytes / f_ms / 1e6:7.0f} {b_ms:8.4f} {3 * nbytes / b_ms / 1e6:7.0f} {c_ms:9.4f} | "
                  f"{t_hip:10.4f} {t_torch:12.4f} {t_torch / t_hip:9.2f}")
            del y, go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("off", "on", "kernels"), default=None, help="(internal) the one measurement this process makes")
    a = ap.parse_args()
    if a.child == "kernels":
        return kernel_pair(a.steps)
    if a.child:
        return layer_mode(a.child == "on", a.steps)
    lines = ["HGT layer fwd+bwd with / without use_norm, ogbn-mag shape (make_mag_like scale 1.0), feat 64 -> 64, 8 heads, fp32; "
             "one process per line, in this order:"]
    for mode in ("off", "on", "on", "off", "kernels"):  # (this process never opens the GPU: each child has it alone)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"child {mode} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        lines += [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
