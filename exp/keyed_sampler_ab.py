"""Sampled mini-batch step with the "sort" and the "keyed" neighbour sampler at the ogbn-mag shape, on one box.

    python exp/keyed_sampler_ab.py [--epochs 40] [--out profiles/r13/keyed_sampler_ab.txt]

First, one process per model that splits the "sort" path's time per batch into its two parts -- the sampling (everything in
``sample_block`` up to the integrated COO) and ``HetGraph.from_integrated_coo`` -- with ``torch.cuda.synchronize()`` + wall clock
around each, as train.py does around the pair, and does the same for the "keyed" path (the four library entries, and
``from_block_separate_coo``).  Then, for each of rgcn, rgat, hgt (hgt with type-sorted runs and full layouts, as train.py asks for):
one process per mode in the order off, on, on, off, each running ``python -m het_amd.train --model M --n_infeat 64 --num_classes
64 --num_layers 2 --batch_size 1024 --fanout 25 20`` (4 heads for rgat and hgt) with or without ``--keyed_sampler`` in-process and
reporting ``minibatch_sample_and_layout_ms`` and the mean forward / backward ms of train.py's protocol.  "off" is method="sort", the
code as it was before the keyed sampler existed."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = ("rgcn", "rgat", "hgt")
STEP_ARGS = ["--n_infeat", "64", "--num_classes", "64", "--num_layers", "2", "--batch_size", "1024", "--fanout", "25", "20"]


def train_mode(model, on, epochs):
    import torch
    from het_amd import train
    res = train.main(["--model", model, "-e", str(epochs), "--num_heads", "4" if model != "rgcn" else "1", *STEP_ARGS]
                     + (["--keyed_sampler"] if on else []))
    print(f"RESULT {model:5s} sampler={'keyed' if on else 'sort '} sample+layout {res['minibatch_sample_and_layout_ms']:8.3f} ms  "
          f"forward {res['mean_forward_ms']:8.4f} ms  backward {res['mean_backward_ms']:8.4f} ms  "
          f"[N={res['num_nodes']} E={res['num_edges']} {epochs} timed steps, {torch.cuda.get_device_name(0)}]")


def split(model, batches):
    """Where a batch's preparation goes, per method: wall clock between synchronisations around the sampling part and the layout
    part of every sample_block call, summed over the two blocks of a batch; mean over `batches` batches after 5 warm-up batches."""
    import torch
    from het_amd import graph, kernels, sampling, train
    dev = torch.device("cuda")
    coo = train.load_graph(argparse.Namespace(edges_npy=None, dataset="mag", scale=1.0))
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    g = graph.HetGraph.from_integrated_coo(coo, full=True)
    N = g.get_num_nodes()
    by_type = model == "hgt"
    acc = {}

    def timed(name, fn):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            acc[name] = acc.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return wrapped

    layouts = {"from_integrated_coo": graph.HetGraph.from_integrated_coo.__func__, "from_block_separate_coo": graph.HetGraph.from_block_separate_coo.__func__}
    for name, fn in layouts.items():
        setattr(graph.HetGraph, name, classmethod(timed(name, fn)))
    for name in ("sample_count", "sample_select", "block_renumber", "block_relation_major"):
        setattr(kernels, name, timed(name, getattr(kernels, name)))
    for method in ("sort", "keyed"):
        s = sampling.NeighborSampler(g, [25, 20], seed=0, full_layouts=by_type, by_type=by_type, method=method)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        edges = nodes = 0
        for i in range(5 + batches):
            if i == 5:
                acc.clear()
                total = 0.0
            seeds = torch.randperm(N, device=dev, generator=gen)[:1024]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blocks = s.sample_blocks(seeds)
            torch.cuda.synchronize()
            if i >= 5:
                total += (time.perf_counter() - t0) * 1e3
                edges += sum(b.graph.get_num_edges() for b in blocks)
                nodes += blocks[0].nodes.numel()
        layout = sum(acc.get(n, 0.0) for n in layouts)
        parts = "  ".join(f"{n} {acc[n] / batches:.3f}" for n in ("sample_count", "sample_select", "block_renumber", "block_relation_major") if n in acc)
        # (the extra synchronisations of the split make `total` larger than train.py's figure for the pair)
        print(f"RESULT split {model:5s} method={method:5s} per batch: total {total / batches:7.3f} ms = sampling {(total - layout) / batches:7.3f} + layouts "
              f"{layout / batches:7.3f} ms  ({edges / batches:.0f} edges, first block {nodes / batches:.0f} nodes; {batches} batches)"
              + (f"  [{parts}]" if parts else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40, help="timed steps per process (train.py's -e)")
    ap.add_argument("--batches", type=int, default=30, help="timed batches of the split")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "keyed_sampler_ab.txt"))
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=MODELS)
    ap.add_argument("--child", default=None, help="(internal) MODEL:on | MODEL:off | MODEL:split: the one measurement this process makes")
    a = ap.parse_args()
    if a.child:
        model, mode = a.child.split(":")
        return split(model, a.batches) if mode == "split" else train_mode(model, mode == "on", a.epochs)
    lines = ["python -m het_amd.train " + " ".join(STEP_ARGS) + " with / without --keyed_sampler, ogbn-mag shape (make_mag_like scale 1.0), "
             "feat 64, fp32; one process per RESULT group, in this order:"]
    print(lines[0], flush=True)
    children = [f"{m}:split" for m in a.models if m != "rgat"] + [f"{m}:{mode}" for m in a.models for mode in ("off", "on", "on", "off")]
    for child in children:
        # (this process never opens the GPU: each child has it alone)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child, "--epochs", str(a.epochs), "--batches", str(a.batches)],
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
