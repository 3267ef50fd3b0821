"""Filtered DistMult ranking (het_amd/linkpred.py distmult_rank, csrc/triple_rank.hip) against its chunked torch composition
(distmult_rank_torch), on one box.

    python exp/rank_ab.py [--reps 200] [--out profiles/r17/rank_ab.txt]

One process, the two forms interleaved, warmed up, HIP events around every repetition: N = 1 939 743 rows of D = 64 (R = 4), fp32 and
bf16, P = 1024 and P = 64 positives drawn by key from the mag-shaped graph, both sides (Q = 2 P), candidates of the true node's type,
filtered on the graph's own edges.  Per shape: the torch composition at three chunk sizes (the best one is the baseline), the native
call whole (pairs, sort, launches), the pair plan (FilterIndex.pairs, with its read-back) apart, the launches alone from the library's
own events with TF of 2 Q N D against the 157.3 TF fp32 matrix peak and TB/s of N D s, and the peak memory of one call.  A form whose
repetition takes more than 10 ms gets a tenth of the repetitions; the counts are printed.  Last, the training script's own
``ranking.ms`` from ``python -m het_amd.train ... --eval_ranking 1024`` in a child process."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNKS = (16384, 65536, 262144)
STEP = ["--model", "rgcn", "--num_layers", "2", "--full_graph_training", "--link_prediction", "--n_infeat", "64", "--num_classes", "64",
        "--batch_size", "1024", "--num_negatives", "1", "-e", "3", "--eval_ranking", "1024"]


def _stats(t):
    if len(t) < 2:
        return t[0], t[0], t[0]
    q = statistics.quantiles(t, n=10)
    return statistics.median(t), q[0], q[-1]


def _fmt(a):
    return f"{a[0]:9.4f} ({a[1]:.4f} .. {a[2]:.4f})"


class _SeparateCoo:
    """The synthetic graph's relation-major COO behind the one call keyed_positive_edges makes."""

    def __init__(self, coo, dev):
        import torch
        ptrs = torch.searchsorted(coo.rel, torch.arange(coo.num_rels + 1))
        self.d = {"rel_ptrs": ptrs.to(dev), "row_indices": coo.row.to(dev), "col_indices": coo.col.to(dev)}

    def get_separate_coo_original(self):
        return self.d


def measure(reps, emit):
    import torch
    import het_amd.kernels as k
    from het_amd import _lib
    from het_amd import linkpred as lp
    from het_amd.synth import make_mag_like
    coo = make_mag_like()
    N, R, D = coo.num_nodes, coo.num_rels, 64
    g = _SeparateCoo(coo, "cuda")
    offs = coo.node_type_offsets.to("cuda")
    F = lp.FilterIndex(coo.row.to("cuda"), coo.rel.to("cuda"), coo.col.to("cuda"), N, R)
    emit(f"filtered ranking, both sides, {reps} repetitions per form (a tenth where one takes more than 10 ms), interleaved; N = {N}, R = {R}, "
         f"D = {D}, node types {offs.tolist()}; {torch.cuda.get_device_name(0)}; library: {_lib.build_info()}; tiles {k.triple_rank_params()}")

    def timed(fn, n):
        ev = []
        for _ in range(n):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            fn()
            e[1].record()
            ev.append(e)
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev]

    def peak_of(fn):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2**20, out

    for P in (1024, 64):
        src, rel, dst = lp.keyed_positive_edges(g, P, seed=0, draw=-1)
        Q = 2 * P
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            torch.manual_seed(0)
            h = (0.5 * torch.randn(N, D, device="cuda")).to(dtype)
            w = 0.5 * torch.randn(R, D, device="cuda")
            kw = dict(sides="both", filter=F, node_type_offsets=offs)
            shape = f"P={P} Q={Q} {name}"
            native = lambda: lp.distmult_rank(h, w, src, rel, dst, **kw)  # noqa: E731
            peak_n, res = peak_of(native)
            m = lp.ranking_metrics(res)
            qa, qr, qt, head = lp._rank_queries(src, rel, dst, "both")
            emit(f"{shape}: pairs {int(F.pairs(qa, qr, head)[0].numel())}, candidates per query {float(res.candidates.float().mean()):.0f}, bad {int(res.bad.sum())}, mrr {m['mrr']:.5f}")
            sweep = {}
            for c in CHUNKS:
                f = lambda c=c: lp.distmult_rank_torch(h, w, src, rel, dst, chunk=c, **kw)  # noqa: E731
                pk, rt = peak_of(f)
                sweep[c] = (_stats(timed(f, 3)), pk)
                assert all(torch.equal(x, y) for x, y in zip(rt[2:], res[2:])), "candidates / bad differ"
                emit(f"{shape} torch chunk {c:7d}: {_fmt(sweep[c][0])} ms over 3 repetitions, peak {pk:9.1f} MiB, "
                     f"greater differs on {int((rt.greater != res.greater).sum())} of {Q} queries")
            best = min(sweep, key=lambda c: sweep[c][0][0])
            torch_f = lambda: lp.distmult_rank_torch(h, w, src, rel, dst, chunk=best, **kw)  # noqa: E731
            n_native = reps
            n_torch = reps if sweep[best][0][0] <= 10.0 else max(3, reps // 10)
            every = max(1, n_native // n_torch)
            for _ in range(5):
                native()
            torch_f()
            tn, tt = [], []
            for i in range(n_native):
                tn += timed(native, 1)
                if i % every == 0 and len(tt) < n_torch:
                    tt += timed(torch_f, 1)
            a, b = _stats(tn), _stats(tt)
            emit(f"{shape} native whole      : {_fmt(a)} ms over {len(tn)} repetitions, peak {peak_n:9.1f} MiB")
            emit(f"{shape} torch chunk {best:7d}: {_fmt(b)} ms over {len(tt)} repetitions, peak {sweep[best][1]:9.1f} MiB (the baseline)")
            emit(f"{shape} native / torch: {a[0] / b[0]:.3f}x of the time")
            plan =_stats(timed(lambda: F.pairs(qa, qr, head), reps))
            pq, pc = F.pairs(qa, qr, head)
            qa, qr, qt = qa.contiguous(), qr.contiguous(), qt.contiguous()
            launches = _stats(timed(lambda: k.triple_rank(h, w, qa, qr, qt, pq, pc, offs), reps))
            _lib.kernel_timing(True)
            for _ in range(reps):
                k.triple_rank(h, w, qa, qr, qt, pq, pc, offs)
            torch.cuda.synchronize()
            (p_ms, p_n), (s_ms, s_n), (r_ms, r_n) = (_lib.kernel_timing_read(n) for n in ("HET_rank_prelude", "HET_rank_pairs", "HET_triple_rank"))
            _lib.kernel_timing(False)
            r1 = r_ms / max(1, r_n)
            emit(f"{shape} pair plan (FilterIndex.pairs, with the read-back) {_fmt(plan)} ms; kernels.triple_rank (workspace, memset, launches) "
                 f"{_fmt(launches)} ms")
            emit(f"{shape} launches alone: prelude {p_ms / max(1, p_n):.4f} ms, pair keys + sort {s_ms / max(1, s_n):.4f} ms, rank pass {r1:.4f} ms = "
                 f"{2.0 * Q * N * D / r1 / 1e9:.1f} TF of 2 Q N D ({100 * 2.0 * Q * N * D / r1 / 1e9 / 157.3:.1f} % of 157.3 TF), "
                 f"{N * D * h.element_size() / r1 / 1e9:.3f} TB/s of N D s = {N * D * h.element_size() / 1e6:.1f} MB")
            del h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_step", action="store_true", help="the interleaved measurement only")
    a = ap.parse_args()
    lines = []

    def emit(line):  # (as it comes: a run of several minutes says where it is)
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    measure(a.reps, emit)
    if not a.skip_step:
        import torch
        torch.cuda.empty_cache()
        r = subprocess.run([sys.executable, "-m", "het_amd.train"] + STEP, capture_output=True, text=True, timeout=600, cwd=ROOT)
        if r.returncode != 0:
            raise SystemExit(f"the training script failed ({r.returncode}):\n{r.stderr[-3000:]}")
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        emit(f"the step: python -m het_amd.train {' '.join(STEP)}")
        emit(f"  ranking {json.dumps(res['ranking'])}  peak_memory_GB {res['peak_memory_GB']:.3f}")


if __name__ == "__main__":
    main()
