"""The row-sparse embedding path without a GPU: the CPU forms of HET_RelGraphEmbed.forward(nodes) (index_select and a cast; dense and
sparse gradient) against index_select / index_add in fp64, RowSparseAdam's composed rule against torch.optim.SparseAdam, the
state_dict moving between the two, and the argument checks of ``het_amd.train --sparse_embed``.  Every test here fails on a tree
without the feature (no het_amd.optim, no forward(nodes), no flag)."""
import pytest
import torch

from tests import _sparse_embed_ref as S
from tests.util import assert_close


def _layer(K, sparse, seed=0):
    from het_amd.layers import HET_RelGraphEmbed
    layer = HET_RelGraphEmbed(S.N, K, sparse=sparse)
    with torch.no_grad():
        layer.embeds.copy_(S.table(K, seed))
    return layer


def test_default_call_is_the_whole_dense_table():
    for sparse in (False, True):
        layer = _layer(32, sparse)
        assert layer() is layer.embeds
        assert list(layer.state_dict()) == ["embeds"]
        layer().sum().backward()
        assert not layer.embeds.grad.is_sparse and torch.equal(layer.embeds.grad, torch.ones(S.N, 32))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("K", S.KS + (10,))
@pytest.mark.parametrize("B", (0, 1, 65, 2049))
def test_forward_and_gradient_on_the_cpu(K, B, sparse):
    """Duplicates in nodes, B = 0: rows and the table's gradient against fp64; the dense gradient is autograd's own, bit for bit."""
    layer = _layer(K, sparse)
    nodes = S.gather_ids(B)
    go = torch.randn(B, K, generator=torch.Generator().manual_seed(B))
    out = layer(nodes)
    assert out.shape == (B, K) and out.dtype == torch.float32 and out.requires_grad
    assert out.grad_fn is not None and out.grad_fn.next_functions[0][0].variable is layer.embeds  # (one node between rows and leaf)
    (outs, gref) = S.dense_ref(layer.embeds, ((nodes, go),))
    assert torch.equal(out.detach().double(), outs[0])
    out.backward(go)
    g = layer.embeds.grad
    if sparse:
        assert g.is_sparse and g._nnz() == B and g._values().dtype == torch.float32
        assert B < 2 or not g.is_coalesced()  # (torch itself marks a tensor of at most one entry coalesced)
        assert torch.equal(g._indices()[0], nodes)
    assert_close(S.grad_dense(layer), gref, what="grad of the table")
    if not sparse and B <= 65:  # (above torch's grain size the CPU index_put_ adds duplicates with atomics: no two runs agree in bits)
        leaf = layer.embeds.detach().clone().requires_grad_(True)
        leaf[nodes].backward(go)
        assert torch.equal(g, leaf.grad)


def test_bf16_rows_and_gradient_on_the_cpu():
    layer = _layer(64, True)
    nodes = S.gather_ids(257)
    out = layer(nodes, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and torch.equal(out, layer.embeds.detach().index_select(0, nodes).to(torch.bfloat16))
    go = torch.randn(257, 64).to(torch.bfloat16)
    out.backward(go)
    assert layer.embeds.grad._values().dtype == torch.float32
    assert_close(S.grad_dense(layer), S.dense_ref(layer.embeds, ((nodes, go),))[1])
    assert layer(None, dtype=torch.bfloat16).dtype == torch.bfloat16  # (no nodes: the whole table, cast)


@pytest.mark.parametrize("sparse", [False, True])
def test_autograd_contract_clauses_on_the_cpu(sparse):
    run_contract_clauses(lambda: _layer(32, sparse), "cpu")


def run_contract_clauses(make_layer, dev):
    """The clauses of tests/_autograd_contract.py that apply to forward(nodes), on ``dev`` (the GPU file runs them too)."""
    K = make_layer().embeds.shape[1]
    gen = torch.Generator().manual_seed(5)
    na, nb = S.gather_ids(65).to(dev), S.gather_ids(257, 1).to(dev)
    ga, gb = torch.randn(65, K, generator=gen), torch.randn(257, K, generator=gen)
    # C2 / C3: one expanded row as grad_out, shared with a residual branch: read, never written, and not kept by the gradient
    layer = make_layer().to(dev)
    row = ga[:1].clone().to(dev)
    god = row.expand(65, K)
    skip = torch.zeros(65, K, device=dev, requires_grad=True)
    out = layer(na)
    (out + skip).backward(god)
    assert torch.equal(row.cpu(), ga[:1]) and torch.equal(skip.grad.cpu(), ga[:1].expand(65, K))
    assert_close(S.grad_dense(layer), S.dense_ref(layer.embeds, ((na, ga[:1].expand(65, K)),))[1], what="expanded grad_out")
    # ... a column slice of a wider tensor
    layer = make_layer().to(dev)
    wide = torch.full((65, K + 8), 7.0)
    wide[:, 4:4 + K] = ga
    wide = wide.to(dev)
    layer(na).backward(wide[:, 4:4 + K])
    assert_close(S.grad_dense(layer), S.dense_ref(layer.embeds, ((na, ga),))[1], what="column-slice grad_out")
    # a contiguous fp32 grad_out that the caller overwrites after the backward: the gradient returned owns its values
    layer = make_layer().to(dev)
    god = ga.clone().to(dev)
    layer(na).backward(god)
    god.fill_(7.0)
    assert_close(S.grad_dense(layer), S.dense_ref(layer.embeds, ((na, ga),))[1], what="grad_out overwritten after the backward")
    # C6: two calls alive before either backward; C7: two backward calls accumulate
    layer = make_layer().to(dev)
    oa = layer(na)
    keep = oa.detach().clone()
    ob = layer(nb)
    ((oa * ga.to(dev)).sum() + (ob * gb.to(dev)).sum()).backward()
    outs, gref = S.dense_ref(layer.embeds, ((na, ga), (nb, gb)))
    assert torch.equal(oa.detach(), keep) and torch.equal(oa.detach().cpu().double(), outs[0]) and torch.equal(ob.detach().cpu().double(), outs[1])
    assert_close(S.grad_dense(layer), gref, what="two calls in one graph")
    layer(na).backward(ga.to(dev))
    assert_close(S.grad_dense(layer), gref + S.dense_ref(layer.embeds, ((na, ga),))[1], what="a second backward accumulates")
    # C4: a frozen table gives no gradient and no graph
    layer = make_layer().to(dev)
    layer.embeds.requires_grad_(False)
    out = layer(na)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out.cpu().double(), outs[0])
    # C8: no_grad / inference_mode calls build no graph; a training step afterwards works
    layer = make_layer().to(dev)
    for mode in (torch.no_grad, torch.inference_mode):
        with mode():
            out = layer(na.clone())
        assert not out.requires_grad and out.grad_fn is None and torch.equal(out.cpu().double(), outs[0])
    layer(na).backward(ga.to(dev))
    assert_close(S.grad_dense(layer), S.dense_ref(layer.embeds, ((na, ga),))[1], what="training step after evaluation")


def test_the_node_saves_the_ids_only():
    layer = _layer(32, True)
    nodes = S.gather_ids(65)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        layer(nodes)
    assert len(saved) == 1 and saved[0].dtype == torch.int64 and torch.equal(saved[0], nodes)


@pytest.mark.parametrize("K", S.KS)
def test_row_sparse_adam_against_sparse_adam_on_the_cpu(K):
    """Three steps on overlapping row sets with duplicates, through nn.Embedding(sparse=True) in fp64 on one side and
    HET_RelGraphEmbed(sparse=True) + RowSparseAdam in fp32 on the other; row 200 is absent from step 2 only, row 201 from every step."""
    from het_amd.optim import RowSparseAdam
    layer = _layer(K, True)
    emb = torch.nn.Embedding(S.N, K, sparse=True).double()
    emb32 = torch.nn.Embedding(S.N, K, sparse=True)
    with torch.no_grad():
        emb.weight.copy_(layer.embeds.double())
        emb32.weight.copy_(layer.embeds)
    opt, ref, ref32 = (RowSparseAdam(layer.parameters(), **S.HYPER), torch.optim.SparseAdam(emb.parameters(), **S.HYPER),
                       torch.optim.SparseAdam(emb32.parameters(), **S.HYPER))
    gen = torch.Generator().manual_seed(K)
    for step in range(3):
        nodes = torch.randint(0, 200, (300,), generator=gen)  # (300 draws of 200 rows: duplicates, and overlap between the steps)
        if step != 1:
            nodes[7] = 200
        go = torch.randn(300, K, generator=gen)
        before = [t[200:202].detach().clone() for t in (layer.embeds, *(opt.state[layer.embeds].get(k, torch.zeros(S.N, K))
                                                                          for k in ("exp_avg", "exp_avg_sq")))]
        for o, rows, g in ((opt, layer(nodes), go), (ref, emb(nodes), go.double()), (ref32, emb32(nodes), go)):
            o.zero_grad()
            (rows * g).sum().backward()
            o.step()
        st = opt.state[layer.embeds]
        assert st["step"] == step + 1 == ref.state[emb.weight]["step"]
        after = [t[200:202].detach() for t in (layer.embeds, st["exp_avg"], st["exp_avg_sq"])]
        for b, a in zip(before, after):
            assert torch.equal(b[1], a[1]), "a row no step names changed"
            assert torch.equal(b[0], a[0]) == (step == 1), "row 200 is absent from step 2 alone"
        for name, d, d32 in zip(("p", "exp_avg", "exp_avg_sq"), S.deviations(opt, layer.embeds, ref, emb.weight),
                                S.deviations(ref32, emb32.weight, ref, emb.weight)):
            print(f"K={K} step {step + 1} {name}: d {d:.3e} d_ref {d32:.3e}")
            assert d <= 2 * d32 + S.FLOOR, (name, step, d, d32)


def test_preset_moments_and_patterns_on_the_cpu():
    """The GPU file's three-step check on CPU tensors (the composed rule): every id pattern at B = 257."""
    from het_amd.optim import RowSparseAdam
    for pattern in ("distinct", "one", "runs"):
        grads = []
        for s in range(3):
            ids, n, coalesced = S.adam_ids(pattern, 257, s)
            grads.append((ids, torch.randn(257, 32, generator=torch.Generator().manual_seed(s)), coalesced))
        S.three_steps(RowSparseAdam, "cpu", 32, grads, n=n, what=pattern)


def test_state_dict_moves_between_the_two_optimizers():
    from het_amd.optim import RowSparseAdam
    K, ids = 32, S.gather_ids(65)
    vals = [torch.randn(65, K, generator=torch.Generator().manual_seed(s)) for s in range(2)]

    def run(first_cls, second_cls):
        p = S.table(K).requires_grad_(True)
        a = first_cls([p], **S.HYPER)
        p.grad = S.sparse_grad(ids, vals[0], p.shape)
        a.step()
        b = second_cls([p], **S.HYPER)
        b.load_state_dict(a.state_dict())
        assert set(b.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and b.state[p]["step"] == 1
        p.grad = S.sparse_grad(ids, vals[1], p.shape)
        b.step()
        return p.detach(), b.state[p]

    results = [run(a, b) for a in (RowSparseAdam, torch.optim.SparseAdam) for b in (RowSparseAdam, torch.optim.SparseAdam)]
    p0, s0 = results[-1]  # SparseAdam alone
    for p, s in results[:-1]:
        assert s["step"] == 2
        torch.testing.assert_close(p, p0, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s["exp_avg"], s0["exp_avg"], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(s["exp_avg_sq"], s0["exp_avg_sq"], rtol=1e-5, atol=1e-7)


def test_skipped_and_refused_gradients():
    from het_amd.optim import RowSparseAdam
    p, q = S.table(8).requires_grad_(True), S.table(8, 1).requires_grad_(True)
    keep = q.detach().clone()
    opt = RowSparseAdam([p, q], lr=0.1)
    p.grad = S.sparse_grad(torch.tensor([3, 3]), torch.ones(2, 8), p.shape)
    v0 = p._version
    opt.step()  # q has no gradient: skipped, no state
    assert torch.equal(q, keep) and len(opt.state[q]) == 0 and opt.state[p]["step"] == 1 and p._version > v0
    p.grad = S.sparse_grad(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 8), p.shape)  # nothing named: only the count advances
    keep = p.detach().clone()
    opt.step()
    assert torch.equal(p, keep) and opt.state[p]["step"] == 2
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="SparseAdam does not support dense gradients, please consider Adam instead"):
        opt.step()
    for bad in (dict(lr=0.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0))):
        with pytest.raises(ValueError):
            RowSparseAdam([p], **bad)
    assert "weight decay" in RowSparseAdam.__doc__ and "dist" in RowSparseAdam.__doc__


@pytest.mark.parametrize("other,word", [("--full_graph_training", "full_graph_training"), ("--inference", "inference")])
def test_train_refuses_sparse_embed_off_the_minibatch_path(other, word):
    from het_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--model", "rgcn", "--scale", "2e-3", "--sparse_embed", other])
    assert "--sparse_embed" in str(e.value) and word in str(e.value)


def test_optimizer_pair_is_two_calls():
    from het_amd import train
    calls = []

    class O:
        def __init__(self, n):
            self.n = n

        def zero_grad(self):
            calls.append(("zero", self.n))

        def step(self):
            calls.append(("step", self.n))

    pair = train.OptimizerPair(O(0), O(1))
    pair.zero_grad()
    pair.step()
    assert calls == [("zero", 0), ("zero", 1), ("step", 0), ("step", 1)]
