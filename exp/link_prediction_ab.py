"""The DistMult link-prediction head (het_amd/linkpred.py DistMultDecoder, csrc/triple_score.hip) against its torch composition
``(h[s] * w[r] * h[o]).sum(-1)``, on one box.

    python exp/link_prediction_ab.py [--reps 200] [--epochs 30] [--out profiles/r16/link_prediction_ab.txt]

1. The decoder alone, one process, the two forms interleaved, warmed up, HIP events around every repetition, forward and backward
   apart: N = 1 939 743 rows of D = 64, fp32 and bf16, positives drawn by key from the mag-shaped graph (so the hubs are real) with keyed
   corruptions: a mini-batch (P = 1024 with K = 1 and K = 16) and a full-graph-scale batch (P = 2^20, K = 1).  Per form: median / p10 /
   p90 in ms and the peak memory of one forward + backward above what was allocated before; for the native form the launches alone
   (the library's own events) with TB/s over 2 T D s + 28 T bytes forward and 4 T D s + N D s + 60 T backward, and ``triple_plan`` on
   its own.  The native forward holds the plan (the sorts), as the autograd node builds it there.
2. The step: ``python -m het_amd.train --model rgcn --num_layers 2 --full_graph_training --link_prediction``, one process per mode in
   the order off, on, on, off; "off" is the same step with DistMultDecoder forced to its torch composition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP = ["--model", "rgcn", "--num_layers", "2", "--full_graph_training", "--link_prediction", "--n_infeat", "64", "--num_classes", "64"]
STEPS = (("rgcn full-graph, P = 1024, K = 1", STEP + ["--batch_size", "1024", "--num_negatives", "1"]),
         ("rgcn full-graph, P = 2^20, K = 1", STEP + ["--batch_size", str(2 ** 20), "--num_negatives", "1"]))


def _stats(t):
    q = statistics.quantiles(t, n=10)
    return statistics.median(t), q[0], q[-1]


class _SeparateCoo:
    """The synthetic graph's relation-major COO behind the one call keyed_positive_edges makes."""

    def __init__(self, coo, dev):
        import torch
        ptrs = torch.searchsorted(coo.rel, torch.arange(coo.num_rels + 1))
        self.d = {"rel_ptrs": ptrs.to(dev), "row_indices": coo.row.to(dev), "col_indices": coo.col.to(dev)}

    def get_separate_coo_original(self):
        return self.d


def alone(reps):
    import torch
    import het_amd.kernels as k
    from het_amd import _lib
    from het_amd.linkpred import DistMultDecoder, keyed_corruptions, keyed_positive_edges, link_prediction_loss
    from het_amd.synth import make_mag_like
    coo = make_mag_like()
    N, R, D = coo.num_nodes, coo.num_rels, 64
    g = _SeparateCoo(coo, "cuda")
    offs = coo.node_type_offsets.to("cuda")
    print(f"RESULT the decoder alone: forward and backward, {reps} repetitions per form, interleaved; N = {N}, R = {R}, D = {D}; "
          f"{torch.cuda.get_device_name(0)}; library: {_lib.build_info()}")
    print(f"RESULT {'batch':22s} {'':5s} {'form':6s} {'fwd ms (p10 .. p90)':>26s} {'bwd ms (p10 .. p90)':>26s} {'peak MiB':>9s}")
    for P, K in ((1024, 1), (1024, 16), (2 ** 20, 1)):
        src, rel, dst = keyed_positive_edges(g, P, seed=0, draw=0)
        s, r, o = keyed_corruptions(src, rel, dst, K, seed=0, draw=1, node_type_offsets=offs, num_nodes=N)
        T = s.shape[0]
        slots = torch.bincount(torch.cat([s, o]), minlength=N)
        batch = f"P={P} K={K} T={T}"
        print(f"RESULT {batch}: most slots on one node {int(slots.max())}, nodes with more than L = {k.triple_long_list()} slots "
              f"{int((slots > k.triple_long_list()).sum())}, nodes with a slot {int((slots > 0).sum())}")
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            torch.manual_seed(0)
            h = (0.5 * torch.randn(N, D, device="cuda")).to(dtype).requires_grad_(True)
            native, comp = DistMultDecoder(R, D).to("cuda"), DistMultDecoder(R, D, native=False).to("cuda")
            with torch.no_grad():
                comp.w_relation.copy_(native.w_relation)
            assert native.takes_native(h) and not comp.takes_native(h)
            forms = {"torch": comp, "native": native}

            def once(f, record):
                h.grad = None
                forms[f].w_relation.grad = None
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                loss = link_prediction_loss(forms[f](h, s, r, o), P)
                e[1].record()
                loss.backward()
                e[2].record()
                if record is not None:
                    record.append(e)
                return loss

            peak, value = {}, {}
            for f in forms:
                value[f] = float(once(f, None))
                h.grad = None
                forms[f].w_relation.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                once(f, None)
                torch.cuda.synchronize()
                peak[f] = (torch.cuda.max_memory_allocated() - base) / 2**20
            for _ in range(10):
                for f in forms:
                    once(f, None)
            ev = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    once(f, ev[f])
            torch.cuda.synchronize()
            times = {}
            for f in forms:
                a, b = _stats([e[0].elapsed_time(e[1]) for e in ev[f]]), _stats([e[1].elapsed_time(e[2]) for e in ev[f]])
                times[f] = (a, b)
                print(f"RESULT {batch:22s} {name:5s} {f:6s} {a[0]:9.4f} ({a[1]:.4f} .. {a[2]:.4f}) {b[0]:9.4f} ({b[1]:.4f} .. {b[2]:.4f}) {peak[f]:9.1f}")
            (tf, tb), (kf, kb) = times["torch"], times["native"]
            print(f"RESULT {batch:22s} {name:5s} native / torch: forward {kf[0] / tf[0]:.2f}x, backward {kb[0] / tb[0]:.2f}x, forward + backward "
                  f"{(kf[0] + kb[0]) / (tf[0] + tb[0]):.2f}x of the time; loss {value['native']:.6f} against {value['torch']:.6f}")
            _lib.kernel_timing(True)  # the launches alone: the library's own events around each entry's launches
            for _ in range(reps):
                once("native", None)
            torch.cuda.synchronize()
            (f_ms, f_n), (p_ms, p_n), (c_ms, c_n), (gh_ms, gh_n), (gw_ms, gw_n) = (_lib.kernel_timing_read(n) for n in (
                "HET_distmult_score", "HET_triple_plan", "HET_distmult_grad_chunks", "HET_distmult_grad_h", "HET_distmult_grad_w"))
            _lib.kernel_timing(False)
            es = h.element_size()
            fb, bb = 2 * T * D * es + 28 * T, 4 * T * D * es + N * D * es + 60 * T
            fwd_ms, plan_ms, bwd_ms = f_ms / max(1, f_n), p_ms / max(1, p_n), (c_ms + gh_ms + gw_ms) / max(1, gh_n)
            print(f"RESULT {batch:22s} {name:5s} native, the launches alone: score {fwd_ms:.4f} ms = {fb / fwd_ms / 1e9:.2f} TB/s of {fb / 1e6:.1f} MB, "
                  f"plan {plan_ms:.4f} ms, backward {bwd_ms:.4f} ms = {bb / bwd_ms / 1e9:.2f} TB/s of {bb / 1e6:.1f} MB (chunk passes "
                  f"{c_ms / max(1, gh_n):.4f}, grad_h {gh_ms / max(1, gh_n):.4f}, grad_w {gw_ms / max(1, gw_n):.4f})")
            pe = []
            for _ in range(reps):  # triple_plan on its own, through its wrapper (allocations included)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                k.triple_plan(s, r, o, N, R)
                e[1].record()
                pe.append(e)
            torch.cuda.synchronize()
            a = _stats([e[0].elapsed_time(e[1]) for e in pe])
            print(f"RESULT {batch:22s} {name:5s} triple_plan alone {a[0]:9.4f} ({a[1]:.4f} .. {a[2]:.4f}) ms")
            del h, native, comp


def step(mode, argv):
    from het_amd import linkpred, train
    if mode == "off":  # the same step on the torch composition
        linkpred.DistMultDecoder.takes_native = lambda self, h: False
    train.main(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_steps", action="store_true", help="part 1 only")
    ap.add_argument("--child", choices=("alone", "on", "off"), default=None, help="(internal) the one measurement this process makes")
    a, rest = ap.parse_known_args()
    if a.child == "alone":
        return alone(a.reps)
    if a.child in ("on", "off"):
        return step(a.child, rest)
    lines = []

    def emit(line):  # (as it comes: a run of several minutes says where it is)
        lines.append(line)
        print(line, flush=True)

    me = [sys.executable, os.path.abspath(__file__)]
    r = subprocess.run(me + ["--child", "alone", "--reps", str(a.reps)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:  # (this process never opens the GPU: each child has it alone)
        raise SystemExit(f"child alone failed ({r.returncode}):\n{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("RESULT "):
            emit(l[len("RESULT "):])
    if not a.skip_steps:
        emit(f"the step: python -m het_amd.train ARGS -e {a.epochs}, one process per line, in this order (off: DistMultDecoder on its torch composition):")
        for what, args in STEPS:
            emit(f"{what}: {' '.join(args)}")
            for mode in ("off", "on", "on", "off"):
                r = subprocess.run(me + ["--child", mode] + args + ["-e", str(a.epochs)], capture_output=True, text=True, timeout=900, cwd=ROOT)
                if r.returncode != 0:
                    raise SystemExit(f"{what} {mode} failed ({r.returncode}):\n{r.stderr[-3000:]}")
                res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                emit(f"  native={mode:3s} forward {res['mean_forward_ms']:.4f} ms  backward {res['mean_backward_ms']:.4f} ms  "
                     f"peak_memory_GB {res['peak_memory_GB']:.3f}  final_loss {res['final_loss']:.6f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
