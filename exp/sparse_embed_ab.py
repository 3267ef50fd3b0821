"""Sampled mini-batch training step with and without --sparse_embed at the ogbn-mag shape, on one box, and the two kernels of
csrc/rows_embed.hip alone at the size of that run's first block.

    python exp/sparse_embed_ab.py [--epochs 40] [--out profiles/r11/sparse_embed_ab.txt]

For each of rgcn, rgat, hgt: one process per mode in the order off, on, on, off, each running
``python -m het_amd.train --model M --n_infeat 64 --num_classes 64 --num_layers 2 --batch_size 1024 --fanout 25 20`` (4 heads for
rgat and hgt) with or without ``--sparse_embed`` in-process and reporting the
mean forward / backward ms of train.py's protocol (5 warm-up steps; the first 3 timed steps, then the first quarter of the rest,
dropped; the optimizer step inside "backward"), the peak memory, and B, the rows of the first sampled block.  Then one process
that times het_rows_embed_gather (fp32 and bf16 rows) and het_rows_adam alone on a table of the graph's size at that B, with the
library's own events around each launch (het_kernel_timing): GB/s of 2 B K 4 bytes (gather; bf16 rows: B K 6) and 7 B K 4 bytes
(Adam: p, m, v read and written, the gradient read)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = ("rgcn", "rgat", "hgt")
STEP_ARGS = ["--n_infeat", "64", "--num_classes", "64", "--num_layers", "2", "--batch_size", "1024", "--fanout", "25", "20"]


def train_mode(model, on, epochs):
    import torch
    from het_amd import sampling, train
    first = []
    sample = sampling.NeighborSampler.sample_blocks

    def recording(self, seeds):
        blocks = sample(self, seeds)
        if not first:
            first.append(blocks[0].nodes.numel())
        return blocks

    sampling.NeighborSampler.sample_blocks = recording
    res = train.main(["--model", model, "-e", str(epochs), "--num_heads", "4" if model != "rgcn" else "1", *STEP_ARGS]
                     + (["--sparse_embed"] if on else []))
    print(f"RESULT {model:5s} sparse_embed={'on ' if on else 'off'} forward {res['mean_forward_ms']:8.4f} ms  backward {res['mean_backward_ms']:8.4f} ms  "
          f"peak memory {res['peak_memory_GB']:.3f} GB  first block B={first[0]}  sample+layout {res['minibatch_sample_and_layout_ms']} ms  "
          f"[N={res['num_nodes']} E={res['num_edges']} {epochs} timed steps, {torch.cuda.get_device_name(0)}]")


def kernels_alone(steps):
    import torch
    from het_amd import _lib, kernels as k, train
    from het_amd.graph import HetGraph
    from het_amd.sampling import NeighborSampler
    dev = torch.device("cuda")
    coo = train.load_graph(argparse.Namespace(edges_npy=None, dataset="mag", scale=1.0))
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    g = HetGraph.from_integrated_coo(coo, full=True)
    N, K = g.get_num_nodes(), 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    seeds = torch.randperm(N, device=dev, generator=gen)[:1024]  # (train.py's first batch)
    nodes = NeighborSampler(g, [25, 20], seed=0, full_layouts=False).sample_blocks(seeds)[0].nodes
    B = nodes.numel()
    distinct = torch.unique(nodes).numel()
    torch.manual_seed(0)
    p, m, v = (torch.randn(N, K, device=dev) for _ in range(3))
    v.abs_()
    grad = torch.randn(B, K, device=dev)
    rows_sorted, perm = torch.sort(nodes, stable=True)
    print(f"RESULT kernels alone: table [{N}, {K}] fp32 ({N * K * 4 / 1e6:.0f} MB), first block B={B} rows ({distinct} distinct), "
          f"{steps} launches each after 10 warm-up launches; library: {_lib.build_info()}")
    cases = (("het_rows_embed_gather", "HET_rows_embed_gather", 2 * B * K * 4, lambda: k.rows_embed_gather(p, nodes)),
             ("het_rows_embed_gather_bf16", "HET_rows_embed_gather", B * K * 6, lambda: k.rows_embed_gather(p, nodes, torch.bfloat16)),
             ("het_rows_adam (perm)", "HET_rows_adam", 7 * B * K * 4, lambda: k.rows_adam_(p, m, v, rows_sorted, perm, grad, 1e-3, 0.9, 0.999, 1e-8, 10)),
             ("het_rows_adam (perm NULL)", "HET_rows_adam", 7 * B * K * 4, lambda: k.rows_adam_(p, m, v, rows_sorted, None, grad, 1e-3, 0.9, 0.999, 1e-8, 10)))
    for name, kernel, nbytes, fn in cases:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        _lib.kernel_timing(True)
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ms, n = _lib.kernel_timing_read(kernel)
        _lib.kernel_timing(False)
        ms /= max(1, n)
        print(f"RESULT {name:28s} {ms * 1e3:8.2f} us  {nbytes / 1e6:7.2f} MB  {nbytes / ms / 1e6:7.0f} GB/s  ({n} launches)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40, help="timed steps per process (train.py's -e)")
    ap.add_argument("--steps", type=int, default=200, help="timed launches per kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "sparse_embed_ab.txt"))
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=MODELS)
    ap.add_argument("--child", default=None, help="(internal) MODEL:on | MODEL:off | kernels: the one measurement this process makes")
    a = ap.parse_args()
    if a.child == "kernels":
        return kernels_alone(a.steps)
    if a.child:
        model, mode = a.child.split(":")
        return train_mode(model, mode == "on", a.epochs)
    lines = ["python -m het_amd.train " + " ".join(STEP_ARGS) + " with / without --sparse_embed, ogbn-mag shape (make_mag_like scale 1.0), "
             "feat 64, fp32; one process per line, in this order:"]
    print(lines[0], flush=True)
    for child in [f"{m}:{mode}" for m in a.models for mode in ("off", "on", "on", "off")] + ["kernels"]:
        # (this process never opens the GPU: each child has it alone)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child, "--epochs", str(a.epochs), "--steps", str(a.steps)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            # a Python error of one configuration is recorded and the rest still measured; anything that may have left the device in
            # a bad state (a signal, a HIP error) ends the run here
            if r.returncode != 1 or "HIP error" in r.stderr or "hipError" in r.stderr:
                raise SystemExit(f"child {child} failed ({r.returncode}):\n{r.stderr[-3000:]}")
            print(r.stderr[-3000:], file=sys.stderr, flush=True)
        new = [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")] or [f"{child}: failed, see stderr"]
        print("\n".join(new), flush=True)
        lines += new
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
