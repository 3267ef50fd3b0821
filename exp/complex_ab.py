"""The ComplEx link-prediction head (het_amd/linkpred.py ComplExDecoder and complex_rank; the ComplExTerms instantiations of
csrc/triple_score.hip and HET_complex_rank_prelude of csrc/triple_rank.hip) against its own torch composition and against the native
DistMult head at the same shapes, on one box.

    python exp/complex_ab.py [--reps 200] [--out profiles/r19/complex_ab.txt]

1. The decoder alone, one process, three forms interleaved (the ComplEx torch composition, native ComplEx, native DistMult as the
   yardstick), warmed up, HIP events around every repetition, forward and backward apart: N = 1 939 743 rows of D = 64 (R = 4), fp32
   and bf16, positives drawn by key from the mag-shaped graph with keyed corruptions: P = 1024 with K = 1 and K = 16, and P = 2^20
   with K = 1.  Per form: median (p10 .. p90) in ms and the peak memory of one forward + backward above what was allocated before;
   for the two native forms the launches alone (the library's own events).  The native forward holds the plan (the sorts), as the
   autograd node builds it there.
2. Filtered ranking, both sides, P = 64 and P = 1024: native complex_rank whole against complex_rank_torch at the best of three chunk
   sizes, and native distmult_rank as the yardstick; the preludes alone from the library's own events.  A form whose repetition takes
   more than 10 ms gets a tenth of the repetitions; the counts are printed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNKS = (16384, 65536, 262144)


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


def score_part(reps, emit, coo, g, offs):
    import torch
    from het_amd import _lib
    from het_amd.linkpred import ComplExDecoder, DistMultDecoder, keyed_corruptions, keyed_positive_edges, link_prediction_loss
    N, R, D = coo.num_nodes, coo.num_rels, 64
    emit(f"the decoder alone: forward and backward, {reps} repetitions per form, three forms interleaved; N = {N}, R = {R}, D = {D}; "
         f"{torch.cuda.get_device_name(0)}; library: {_lib.build_info()}")
    emit(f"{'batch':22s} {'':5s} {'form':9s} {'fwd ms (p10 .. p90)':>26s} {'bwd ms (p10 .. p90)':>26s} {'peak MiB':>9s}")
    for P, K in ((1024, 1), (1024, 16), (2 ** 20, 1)):
        src, rel, dst = keyed_positive_edges(g, P, seed=0, draw=0)
        s, r, o = keyed_corruptions(src, rel, dst, K, seed=0, draw=1, node_type_offsets=offs, num_nodes=N)
        T = s.shape[0]
        batch = f"P={P} K={K} T={T}"
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            torch.manual_seed(0)
            h = (0.5 * torch.randn(N, D, device="cuda")).to(dtype).requires_grad_(True)
            forms = {"torch": ComplExDecoder(R, D, native=False).to("cuda"), "complex": ComplExDecoder(R, D).to("cuda"),
                     "distmult": DistMultDecoder(R, D).to("cuda")}
            with torch.no_grad():
                for f in ("torch", "distmult"):
                    forms[f].w_relation.copy_(forms["complex"].w_relation)
            assert forms["complex"].takes_native(h) and forms["distmult"].takes_native(h) and not forms["torch"].takes_native(h)

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
                emit(f"{batch:22s} {name:5s} {f:9s} {_fmt(a)} {_fmt(b)} {peak[f]:9.1f}")
            (tf, tb), (kf, kb), (df, db) = times["torch"], times["complex"], times["distmult"]
            emit(f"{batch:22s} {name:5s} complex / torch: forward {kf[0] / tf[0]:.2f}x, backward {kb[0] / tb[0]:.2f}x, forward + backward "
                 f"{(kf[0] + kb[0]) / (tf[0] + tb[0]):.2f}x of the time; loss {value['complex']:.6f} against {value['torch']:.6f}")
            emit(f"{batch:22s} {name:5s} complex / distmult: forward {kf[0] / df[0]:.2f}x, backward {kb[0] / db[0]:.2f}x, forward + backward "
                 f"{(kf[0] + kb[0]) / (df[0] + db[0]):.2f}x of the time")
            es = h.element_size()
            fb, bb = 2 * T * D * es + 28 * T, 4 * T * D * es + N * D * es + 60 * T
            for f, pre in (("complex", "HET_complex"), ("distmult", "HET_distmult")):
                _lib.kernel_timing(True)  # the launches alone: the library's own events around each entry's launches
                for _ in range(reps):
                    once(f, None)
                torch.cuda.synchronize()
                (f_ms, f_n), (c1_ms, _), (c2_ms, _), (gh_ms, gh_n), (gw_ms, gw_n) = (_lib.kernel_timing_read(pre + n) for n in (
                    "_score", "_grad_chunks_h", "_grad_chunks_w", "_grad_h", "_grad_w"))
                _lib.kernel_timing(False)
                fwd_ms, bwd_ms = f_ms / max(1, f_n), (c1_ms + c2_ms + gh_ms + gw_ms) / max(1, gh_n)
                emit(f"{batch:22s} {name:5s} {f}, the launches alone: score {fwd_ms:.4f} ms = {fb / fwd_ms / 1e9:.2f} TB/s of {fb / 1e6:.1f} MB, "
                     f"backward {bwd_ms:.4f} ms = {bb / bwd_ms / 1e9:.2f} TB/s of {bb / 1e6:.1f} MB (chunk passes "
                     f"{(c1_ms + c2_ms) / max(1, gh_n):.4f}, grad_h {gh_ms / max(1, gh_n):.4f}, grad_w {gw_ms / max(1, gw_n):.4f})")
            del h, forms


def rank_part(reps, emit, coo, g, offs):
    import torch
    import het_amd.kernels as k
    from het_amd import _lib
    from het_amd import linkpred as lp
    N, R, D = coo.num_nodes, coo.num_rels, 64
    F = lp.FilterIndex(coo.row.to("cuda"), coo.rel.to("cuda"), coo.col.to("cuda"), N, R)
    emit(f"filtered ranking, both sides, {reps} repetitions per form (a tenth where one takes more than 10 ms), interleaved; N = {N}, R = {R}, "
         f"D = {D}, node types {offs.tolist()}; tiles {k.triple_rank_params()}")

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

    for P in (64, 1024):
        src, rel, dst = lp.keyed_positive_edges(g, P, seed=0, draw=-1)
        Q = 2 * P
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            torch.manual_seed(0)
            h = (0.5 * torch.randn(N, D, device="cuda")).to(dtype)
            w = 0.5 * torch.randn(R, D, device="cuda")
            kw = dict(sides="both", filter=F, node_type_offsets=offs)
            shape = f"P={P} Q={Q} {name}"
            native = lambda: lp.complex_rank(h, w, src, rel, dst, **kw)  # noqa: E731
            yard = lambda: lp.distmult_rank(h, w, src, rel, dst, **kw)  # noqa: E731
            peak_n, res = peak_of(native)
            m = lp.ranking_metrics(res)
            emit(f"{shape}: candidates per query {float(res.candidates.float().mean()):.0f}, bad {int(res.bad.sum())}, mrr {m['mrr']:.5f}; tail and "
                 f"head counts differ on {int((res.greater[:P] != res.greater[P:]).sum())} of {P} triples")
            sweep = {}
            for c in CHUNKS:
                f = lambda c=c: lp.complex_rank_torch(h, w, src, rel, dst, chunk=c, **kw)  # noqa: E731
                pk, rt = peak_of(f)
                sweep[c] = (_stats(timed(f, 3)), pk)
                assert all(torch.equal(x, y) for x, y in zip(rt[2:], res[2:])), "candidates / bad differ"
                emit(f"{shape} torch chunk {c:7d}: {_fmt(sweep[c][0])} ms over 3 repetitions, peak {pk:9.1f} MiB, "
                     f"greater differs on {int((rt.greater != res.greater).sum())} of {Q} queries")
            best = min(sweep, key=lambda c: sweep[c][0][0])
            torch_f = lambda: lp.complex_rank_torch(h, w, src, rel, dst, chunk=best, **kw)  # noqa: E731
            n_torch = reps if sweep[best][0][0] <= 10.0 else max(3, reps // 10)
            every = max(1, reps // n_torch)
            for _ in range(5):
                native()
                yard()
            torch_f()
            tn, ty, tt = [], [], []
            for i in range(reps):
                tn += timed(native, 1)
                ty += timed(yard, 1)
                if i % every == 0 and len(tt) < n_torch:
                    tt += timed(torch_f, 1)
            a, y, b = _stats(tn), _stats(ty), _stats(tt)
            emit(f"{shape} complex whole     : {_fmt(a)} ms over {len(tn)} repetitions, peak {peak_n:9.1f} MiB")
            emit(f"{shape} distmult whole    : {_fmt(y)} ms over {len(ty)} repetitions (the yardstick)")
            emit(f"{shape} torch chunk {best:7d}: {_fmt(b)} ms over {len(tt)} repetitions, peak {sweep[best][1]:9.1f} MiB (the baseline)")
            emit(f"{shape} complex / torch: {a[0] / b[0]:.3f}x of the time; complex / distmult: {a[0] / y[0]:.3f}x of the time")
            _lib.kernel_timing(True)
            for _ in range(reps):
                native()
                yard()
            torch.cuda.synchronize()
            (c_ms, c_n), (p_ms, p_n), (r_ms, r_n) = (_lib.kernel_timing_read(n) for n in ("HET_complex_rank_prelude", "HET_rank_prelude", "HET_triple_rank"))
            _lib.kernel_timing(False)
            emit(f"{shape} launches alone: complex prelude {c_ms / max(1, c_n):.4f} ms, distmult prelude {p_ms / max(1, p_n):.4f} ms, rank pass "
                 f"{r_ms / max(1, r_n):.4f} ms (both heads, {r_n} launches)")
            del h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_rank", action="store_true", help="part 1 only")
    ap.add_argument("--skip_score", action="store_true", help="part 2 only")
    a = ap.parse_args()
    lines = []

    def emit(line):  # (as it comes: a run of several minutes says where it is)
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    from het_amd.synth import make_mag_like
    coo = make_mag_like()
    g = _SeparateCoo(coo, "cuda")
    offs = coo.node_type_offsets.to("cuda")
    if not a.skip_score:
        score_part(a.reps, emit, coo, g, offs)
    if not a.skip_rank:
        rank_part(a.reps, emit, coo, g, offs)


if __name__ == "__main__":
    main()
