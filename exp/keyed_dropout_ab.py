"""Keyed dropout (het_amd/layers.py KeyedDropout, csrc/keyed_dropout.hip) against the torch pair it replaces, on one box.

    python exp/keyed_dropout_ab.py [--reps 200] [--epochs 30] [--out profiles/r14/keyed_dropout_ab.txt]

1. The pair alone, one process, the two forms interleaved, warmed up, HIP events around every repetition: ``F.dropout(F.relu(y))``
   forward + backward against ``KeyedDropout(0.5, "relu")`` at [1 939 743, 64] fp32 and bf16 (the hidden layers of ogbn-mag) and at
   [1 939 743, 8] fp32 (the logits of the last layer).  Per form: median / p10 / p90 of forward and backward in ms, TB/s of
   2 n s bytes (forward) and 3 n s bytes (backward), and the peak memory of one forward + backward above what was allocated before.
2. The step: ``python -m het_amd.train --model M --num_layers 2 --full_graph_training`` for M = rgat, rgcn, with and without
   ``--keyed_dropout``, one process per mode in the order off, on, on, off: forward, backward and peak_memory_GB of its log line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_MAG = 1939743


def _stats(t):
    q = statistics.quantiles(t, n=10)
    return statistics.median(t), q[0], q[-1]


def pair(reps):
    import torch
    import torch.nn.functional as F
    from het_amd import _lib
    from het_amd.layers import KeyedDropout
    print(f"RESULT the pair alone: relu + dropout 0.5, forward + backward, {reps} repetitions per form, interleaved; {torch.cuda.get_device_name(0)}; "
          f"library: {_lib.build_info()}")
    print(f"RESULT {'shape':14s} {'rows':5s} {'form':6s} {'fwd ms (p10 .. p90)':>26s} {'TB/s':>6s} {'bwd ms (p10 .. p90)':>26s} {'TB/s':>6s} {'peak MiB':>9s}")
    for X, dtype, name in ((64, torch.float32, "fp32"), (64, torch.bfloat16, "bf16"), (8, torch.float32, "fp32")):
        torch.manual_seed(0)
        y = torch.randn(N_MAG, X, device="cuda").to(dtype).requires_grad_(True)
        go = torch.randn(N_MAG, X, device="cuda").to(dtype)
        keyed = KeyedDropout(0.5, "relu", seed=1).cuda()
        forms = {"torch": lambda: F.dropout(F.relu(y), 0.5, True), "keyed": lambda: keyed(y)}
        times = {k: ([], []) for k in forms}
        peak = {}

        def once(k, record):
            y.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            out = forms[k]()
            e[1].record()
            out.backward(go)
            e[2].record()
            if record is not None:
                record.append(e)

        for k in forms:  # peak memory of one forward + backward
            once(k, None)
            y.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            once(k, None)
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base) / 2**20
        for _ in range(10):
            for k in forms:
                once(k, None)
        ev = {k: [] for k in forms}
        for _ in range(reps):
            for k in forms:
                once(k, ev[k])
        torch.cuda.synchronize()
        nbytes = y.numel() * y.element_size()
        for k in forms:
            f, b = _stats([e[0].elapsed_time(e[1]) for e in ev[k]]), _stats([e[1].elapsed_time(e[2]) for e in ev[k]])
            times[k] = (f, b)
            print(f"RESULT [{N_MAG}, {X:2d}] {name:5s} {k:6s} {f[0]:9.4f} ({f[1]:.4f} .. {f[2]:.4f}) {2 * nbytes / f[0] / 1e9:6.2f} "
                  f"{b[0]:9.4f} ({b[1]:.4f} .. {b[2]:.4f}) {3 * nbytes / b[0] / 1e9:6.2f} {peak[k]:9.1f}")
        (tf, tb), (kf, kb) = times["torch"], times["keyed"]
        print(f"RESULT [{N_MAG}, {X:2d}] {name:5s} keyed / torch: forward {kf[0] / tf[0]:.2f}x, backward {kb[0] / tb[0]:.2f}x, "
              f"forward + backward {(kf[0] + kb[0]) / (tf[0] + tb[0]):.2f}x of the time")
        _lib.kernel_timing(True)  # the two launches alone: the library's own events around each, no host time between them
        for _ in range(reps):
            once("keyed", None)
        torch.cuda.synchronize()
        (a_ms, a_n), (b_ms, b_n) = (_lib.kernel_timing_read(k) for k in ("HET_keyed_dropout", "HET_keyed_dropout_backward"))  # (a prefix match)
        _lib.kernel_timing(False)
        f_ms, b_ms = (a_ms - b_ms) / max(1, a_n - b_n), b_ms / max(1, b_n)
        print(f"RESULT [{N_MAG}, {X:2d}] {name:5s} keyed, the launches alone: forward {f_ms:.4f} ms = {2 * nbytes / f_ms / 1e9:.2f} TB/s, "
              f"backward {b_ms:.4f} ms = {3 * nbytes / b_ms / 1e9:.2f} TB/s")
        del y, go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_steps", action="store_true", help="part 1 only")
    ap.add_argument("--child", choices=("pair",), default=None, help="(internal) the one measurement this process makes")
    a = ap.parse_args()
    if a.child == "pair":
        return pair(a.reps)
    lines = []
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "pair", "--reps", str(a.reps)], capture_output=True, text=True,
                       timeout=900)  # (this process never opens the GPU: each child has it alone)
    if r.returncode != 0:
        raise SystemExit(f"child pair failed ({r.returncode}):\n{r.stderr[-3000:]}")
    lines += [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if not a.skip_steps:
        lines.append(f"the step: python -m het_amd.train --model M --num_layers 2 --full_graph_training -e {a.epochs} [--keyed_dropout], "
                     "one process per line, in this order:")
        for model in ("rgat", "rgcn"):
            for mode in ("off", "on", "on", "off"):
                cmd = [sys.executable, "-m", "het_amd.train", "--model", model, "--num_layers", "2", "--full_graph_training", "-e", str(a.epochs)]
                r = subprocess.run(cmd + (["--keyed_dropout"] if mode == "on" else []), capture_output=True, text=True, timeout=900, cwd=ROOT)
                if r.returncode != 0:
                    raise SystemExit(f"{model} {mode} failed ({r.returncode}):\n{r.stderr[-3000:]}")
                res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                lines.append(f"{model} keyed_dropout={mode:3s} forward {res['mean_forward_ms']:.4f} ms  backward {res['mean_backward_ms']:.4f} ms  "
                             f"peak_memory_GB {res['peak_memory_GB']:.3f}  final_loss {res['final_loss']:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
