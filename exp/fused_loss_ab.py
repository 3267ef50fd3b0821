"""The fused softmax cross-entropy (het_amd/layers.py SoftmaxCrossEntropy, csrc/softmax_xent.hip) against the torch expression of the
training script that it replaces, on one box.

    python exp/fused_loss_ab.py [--reps 200] [--epochs 30] [--out profiles/r15/fused_loss_ab.txt]

1. The loss alone, one process, the two forms interleaved, warmed up, HIP events around every repetition, forward and backward apart:
   ``-logits.float().log_softmax(-1).gather(1, labels.view(-1, 1)).mean()`` against ``SoftmaxCrossEntropy()(logits, labels)`` at
   [1 939 743, 8] fp32 (the benchmark's logits), [1 939 743, 349] fp32 and bf16 (ogbn-mag's class count) and [1024, 8] / [1024, 349] fp32
   (a sampled mini-batch).  Per form: median / p10 / p90 in ms and the peak memory of one forward + backward above what was
   allocated before; for the fused form the launches alone (the library's own events) and their TB/s over the bytes each pass has
   to move: N C s + 12 N forward (the logits, a label, an lse), 2 N C s + 12 N backward (s = bytes per logit).
2. The step: ``python -m het_amd.train`` with and without ``--fused_loss``, one process per mode in the order off, on, on, off: RGAT
   full-graph at 8 classes and at 349, and RGAT on sampled mini-batches."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_MAG = 1939743
STEPS = (("rgat full-graph, 8 classes", ["--model", "rgat", "--num_layers", "2", "--full_graph_training"]),
         ("rgat full-graph, 349 classes", ["--model", "rgat", "--num_layers", "2", "--full_graph_training", "--num_classes", "349"]),
         ("rgat sampled, batch 1024, fanout 25 20, 349 classes", ["--model", "rgat", "--num_layers", "2", "--num_classes", "349"]))


def _stats(t):
    q = statistics.quantiles(t, n=10)
    return statistics.median(t), q[0], q[-1]


def alone(reps):
    import torch
    from het_amd import _lib
    from het_amd.layers import SoftmaxCrossEntropy
    print(f"RESULT the loss alone: forward and backward, {reps} repetitions per form, interleaved; {torch.cuda.get_device_name(0)}; "
          f"library: {_lib.build_info()}")
    print(f"RESULT {'shape':15s} {'':5s} {'form':6s} {'fwd ms (p10 .. p90)':>26s} {'bwd ms (p10 .. p90)':>26s} {'peak MiB':>9s}")
    for N, C, dtype, name in ((N_MAG, 8, torch.float32, "fp32"), (N_MAG, 349, torch.float32, "fp32"), (N_MAG, 349, torch.bfloat16, "bf16"),
                              (1024, 8, torch.float32, "fp32"), (1024, 349, torch.float32, "fp32")):
        torch.manual_seed(0)
        z = torch.randn(N, C, device="cuda").to(dtype).requires_grad_(True)
        lab = torch.randint(0, C, (N,), device="cuda")
        fused = SoftmaxCrossEntropy()
        forms = {"torch": lambda: -z.float().log_softmax(dim=-1).gather(1, lab.view(-1, 1)).mean(), "fused": lambda: fused(z, lab)}
        shape = f"[{N}, {C}]"

        def once(k, record):
            z.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            loss = forms[k]()
            e[1].record()
            loss.backward()
            e[2].record()
            if record is not None:
                record.append(e)
            return loss

        peak, value = {}, {}
        for k in forms:  # peak memory of one forward + backward, and the value
            value[k] = float(once(k, None))
            z.grad = None
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
        times = {}
        for k in forms:
            f, b = _stats([e[0].elapsed_time(e[1]) for e in ev[k]]), _stats([e[1].elapsed_time(e[2]) for e in ev[k]])
            times[k] = (f, b)
            print(f"RESULT {shape:15s} {name:5s} {k:6s} {f[0]:9.4f} ({f[1]:.4f} .. {f[2]:.4f}) {b[0]:9.4f} ({b[1]:.4f} .. {b[2]:.4f}) {peak[k]:9.1f}")
        (tf, tb), (kf, kb) = times["torch"], times["fused"]
        print(f"RESULT {shape:15s} {name:5s} fused / torch: forward {kf[0] / tf[0]:.2f}x, backward {kb[0] / tb[0]:.2f}x, forward + backward "
              f"{(kf[0] + kb[0]) / (tf[0] + tb[0]):.2f}x of the time; loss {value['fused']:.6f} against {value['torch']:.6f}")
        _lib.kernel_timing(True)  # the launches alone: the library's own events around each, no host time between them
        for _ in range(reps):
            once("fused", None)
        torch.cuda.synchronize()
        (a_ms, a_n), (f_ms, f_n), (b_ms, b_n) = (_lib.kernel_timing_read(k) for k in ("HET_softmax_xent", "HET_softmax_xent_finish",
                                                                                     "HET_softmax_xent_backward"))  # (a prefix match)
        _lib.kernel_timing(False)
        fwd_ms, fin_ms, bwd_ms = (a_ms - f_ms - b_ms) / max(1, a_n - f_n - b_n), f_ms / max(1, f_n), b_ms / max(1, b_n)
        s = z.element_size()
        fb, bb = N * C * s + 12 * N, 2 * N * C * s + 12 * N
        print(f"RESULT {shape:15s} {name:5s} fused, the launches alone: forward {fwd_ms:.4f} ms = {fb / fwd_ms / 1e9:.2f} TB/s of {fb / 1e6:.1f} MB "
              f"(+ finish {fin_ms:.4f} ms), backward {bwd_ms:.4f} ms = {bb / bwd_ms / 1e9:.2f} TB/s of {bb / 1e6:.1f} MB")
        del z, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_steps", action="store_true", help="part 1 only")
    ap.add_argument("--child", choices=("alone",), default=None, help="(internal) the one measurement this process makes")
    a = ap.parse_args()
    if a.child == "alone":
        return alone(a.reps)
    lines = []

    def emit(line):  # (as it comes: a run of several minutes says where it is)
        lines.append(line)
        print(line, flush=True)

    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "alone", "--reps", str(a.reps)], capture_output=True, text=True,
                       timeout=900)  # (this process never opens the GPU: each child has it alone)
    if r.returncode != 0:
        raise SystemExit(f"child alone failed ({r.returncode}):\n{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("RESULT "):
            emit(l[len("RESULT "):])
    if not a.skip_steps:
        emit(f"the step: python -m het_amd.train ARGS -e {a.epochs} [--fused_loss], one process per line, in this order:")
        for what, args in STEPS:
            emit(f"{what}: {' '.join(args)}")
            for mode in ("off", "on", "on", "off"):
                cmd = [sys.executable, "-m", "het_amd.train"] + args + ["-e", str(a.epochs)]
                r = subprocess.run(cmd + (["--fused_loss"] if mode == "on" else []), capture_output=True, text=True, timeout=900, cwd=ROOT)
                if r.returncode != 0:
                    raise SystemExit(f"{what} {mode} failed ({r.returncode}):\n{r.stderr[-3000:]}")
                res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                emit(f"  fused_loss={mode:3s} forward {res['mean_forward_ms']:.4f} ms  backward {res['mean_backward_ms']:.4f} ms  "
                             f"peak_memory_GB {res['peak_memory_GB']:.3f}  final_loss {res['final_loss']:.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
