"""Shapes, inputs and fp64 references shared by tests/test_sparse_embed_ref.py (CPU) and tests/test_gpu_sparse_embed.py (GPU): the
row gather of HET_RelGraphEmbed.forward(nodes), its dense and sparse gradients, and RowSparseAdam against torch.optim.SparseAdam.

No GPU import here: a device is an argument."""
import torch

N = 257
KS = (4, 32, 64, 68, 256)
B_LADDER = (0, 1, 63, 64, 65, 257, 2049)
RUN_LENGTHS = (1, 2, 63, 64, 65)
FLOOR = 2.0 ** -21  # four fp32 ulps of the largest element: for the cases where torch's own fp32 result happens to be exact


def span(K):
    """Sorted positions one workgroup of csrc/rows_embed.hip covers in its first pass: 256 lanes over lane groups of the smallest
    power of two >= K / 4 lanes (64 at most)."""
    lanes = 1
    while lanes < 64 and lanes < K // 4:
        lanes *= 2
    return 256 // lanes


def table(K, seed=0, n=N):
    return torch.randn(n, K, generator=torch.Generator().manual_seed(1000 + seed))


def gather_ids(B, seed=0):
    """B row ids of [0, N) holding row N - 1 (B >= 1), row 0 (B >= 2) and a repeated id (B >= 3)."""
    ids = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(2000 + seed + B))
    if B >= 1:
        ids[B // 2] = N - 1
    if B >= 2:
        ids[0] = 0
    if B >= 3:
        ids[B - 1] = ids[1]
    return ids


def adam_ids(pattern, B, seed=0):
    """(ids [B] in gradient order, table rows, coalesced) of one id pattern:
    "distinct"  B different rows, ascending: a coalesced gradient (the table has max(N, B + 7) rows: 2049 ids need more than 257)
    "one"       B copies of one row: a run longer than any workgroup's span
    "runs"      runs of 1, 2, 63, 64, 65 equal ids, repeated to B positions, their order in the gradient shuffled (uncoalesced)."""
    gen = torch.Generator().manual_seed(3000 + seed + B)
    if pattern == "distinct":
        n = max(N, B + 7)
        return torch.sort(torch.randperm(n, generator=gen)[:B]).values, n, True
    if pattern == "one":
        return torch.full((B,), 101, dtype=torch.int64), N, False
    assert pattern == "runs"
    lengths = []
    while sum(lengths) < B:
        lengths.append(min(RUN_LENGTHS[len(lengths) % len(RUN_LENGTHS)], B - sum(lengths)))
    rows = torch.sort(torch.randperm(N, generator=gen)[:len(lengths)]).values
    ids = torch.repeat_interleave(rows, torch.tensor(lengths, dtype=torch.int64))
    return ids[torch.randperm(B, generator=gen)], N, False


def runs_cross_spans(ids, K):
    """Whether some run of the sorted ids has positions on both sides of a boundary between two workgroups' spans."""
    s = torch.sort(ids).values
    g = span(K)
    pos = torch.arange(1, s.numel())
    return bool(((s[1:] == s[:-1]) & (pos % g == 0)).any())


def sparse_grad(ids, vals, shape, coalesced=False):
    return torch.sparse_coo_tensor(ids.view(1, -1), vals, shape, is_coalesced=True if coalesced else None)


def start_state(n, K, seed=0):
    """(p, exp_avg, exp_avg_sq) fp32 with recognisable non-zero moments (exp_avg_sq > 0)."""
    gen = torch.Generator().manual_seed(4000 + seed)
    p = torch.randn(n, K, generator=gen)
    m = 0.125 + 0.5 * torch.randn(n, K, generator=gen)
    v = 0.25 + torch.rand(n, K, generator=gen)
    return p, m, v


def make_optimizer(cls, p, m, v, **kw):
    """``cls`` over the leaf ``p`` with its moments preset to copies of m, v (step 0)."""
    opt = cls([p], **kw)
    opt.state[p] = {"step": 0, "exp_avg": m.detach().clone().to(p), "exp_avg_sq": v.detach().clone().to(p)}
    return opt


def deviations(opt, p, ref_opt, ref_p):
    """d = max|x - x64| / max|x64| for x in (p, exp_avg, exp_avg_sq)."""
    out = []
    for x, x64 in ((p, ref_p), (opt.state[p]["exp_avg"], ref_opt.state[ref_p]["exp_avg"]),
                   (opt.state[p]["exp_avg_sq"], ref_opt.state[ref_p]["exp_avg_sq"])):
        x64 = x64.detach().cpu().double()
        out.append(float((x.detach().cpu().double() - x64).abs().max() / x64.abs().max()))
    return out


HYPER = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8)


def three_steps(make_ours, dev, K, grads, n=N, seed=0, what=""):
    """Three consecutive steps on the gradients ``grads`` ((ids, vals fp32 [B,K], coalesced) per step) by ``make_ours`` (RowSparseAdam)
    and by torch.optim.SparseAdam in fp32, both on ``dev``, and by SparseAdam in fp64 on the CPU; after every step
    d_ours <= 2 * d_ref + 2^-21 for p, exp_avg and exp_avg_sq.  Returns the worst (d_ours, d_ref) pair by d_ours."""
    p0, m0, v0 = start_state(n, K, seed)
    def mk(cls, dt, d):
        leaf = p0.detach().clone().to(dt).to(d).requires_grad_(True)
        return leaf, make_optimizer(cls, leaf, m0, v0, **HYPER)

    (p, opt), (pr, ref) = mk(make_ours, torch.float32, dev), mk(torch.optim.SparseAdam, torch.float32, dev)
    p64, ref64 = mk(torch.optim.SparseAdam, torch.float64, "cpu")
    worst = (0.0, 0.0)
    for step, (ids, vals, coalesced) in enumerate(grads):
        for leaf, o, dt, d in ((p, opt, torch.float32, dev), (pr, ref, torch.float32, dev), (p64, ref64, torch.float64, "cpu")):
            leaf.grad = sparse_grad(ids.to(d), vals.to(dt).to(d), leaf.shape, coalesced)
            o.step()
        for name, d_ours, d_ref in zip(("p", "exp_avg", "exp_avg_sq"), deviations(opt, p, ref64, p64), deviations(ref, pr, ref64, p64)):
            print(f"{what} K={K} step {step + 1} {name}: d_ours {d_ours:.3e} d_ref {d_ref:.3e}")
            assert d_ours <= 2 * d_ref + FLOOR, f"{what} K={K} step {step + 1} {name}: {d_ours:.3e} > 2 * {d_ref:.3e} + 2^-21"
            if d_ours > worst[0]:
                worst = (d_ours, d_ref)
        assert opt.state[p]["step"] == step + 1
    return worst


# ---- the clauses of tests/_autograd_contract.py that apply to forward(nodes): there is no graph and one leaf, so they are written
# out here against index_select / index_add in fp64
def dense_ref(embeds, calls):
    """fp64 (outs, grad of the table) of calls ((nodes, go), ...) made in one autograd graph."""
    e64 = embeds.detach().cpu().double()
    grad = torch.zeros_like(e64)
    outs = []
    for nodes, go in calls:
        outs.append(e64.index_select(0, nodes.cpu()))
        grad.index_add_(0, nodes.cpu(), go.detach().cpu().double())
    return outs, grad


def grad_dense(layer):
    g = layer.embeds.grad
    assert g is not None and g.is_sparse == layer.sparse and g.dtype == torch.float32 and g.shape == layer.embeds.shape
    return g.to_dense() if g.is_sparse else g
