"""The row-sparse embedding path on the GPU (csrc/rows_embed.hip): the gather of HET_RelGraphEmbed.forward(nodes), its dense and sparse
gradients, RowSparseAdam's one-launch step against torch.optim.SparseAdam, and ``het_amd.train --sparse_embed`` end to end.

The Adam bound: with d = max|x - x64| / max|x64| for x in (p, exp_avg, exp_avg_sq) against torch.optim.SparseAdam in fp64 on the CPU,
d_hip of the kernel <= 2 * d_ref + 2^-21, d_ref being torch.optim.SparseAdam in fp32 on the same device: twice the error of an equally
valid fp32 evaluation order (README, RGAT bf16 rows), over a floor of four fp32 ulps for the cases where torch's result is exact.
Every test here fails on a tree without the feature."""
import math
import re

import pytest
import torch

from tests import _sparse_embed_ref as S
from tests._poison import POISON_IDS, POISONS, poisoned
from tests.test_sparse_embed_ref import run_contract_clauses
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(K, sparse, seed=0, n=S.N):
    from het_amd.layers import HET_RelGraphEmbed
    layer = HET_RelGraphEmbed(n, K, sparse=sparse)
    with torch.no_grad():
        layer.embeds.copy_(S.table(K, seed, n))
    return layer.to(DEV)


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("K", S.KS + (10, 1024))
def test_gather_on_the_ladder(K):
    """fp32 rows bit for bit index_select, bf16 rows bit for bit its cast; K = 10 takes the fallback and agrees too."""
    import het_amd.kernels as k
    layer = _layer(K, False)
    assert k.rows_embed_ok(K) == (K != 10)
    with torch.no_grad():
        for B in S.B_LADDER:
            nodes = S.gather_ids(B).to(DEV)
            if B >= 3:
                assert {0, S.N - 1} <= set(nodes.tolist()) and nodes.unique().numel() < B
            ref = layer.embeds.index_select(0, nodes)
            for dtype, want in ((None, ref), (torch.float32, ref), (torch.bfloat16, ref.to(torch.bfloat16))):
                out = layer(nodes, dtype=dtype)
                assert out.shape == (B, K) and out.dtype == want.dtype and out.is_contiguous()
                assert torch.equal(out, want), (K, B, dtype)
        strided = torch.stack([nodes, nodes], 1)[:, 0]  # (ids that are no contiguous list)
        assert not strided.is_contiguous() and torch.equal(layer(strided), ref)


def test_gather_falls_back_for_a_table_the_kernel_does_not_take():
    """A non-contiguous table (a column slice) and a float64 output: index_select and a cast, the same values."""
    from het_amd import layers
    wide = S.table(72).to(DEV)
    view = wide[:, 4:68]
    nodes = S.gather_ids(65).to(DEV)
    assert not layers._embed_rows_kernel_ok(view, nodes, torch.float32)
    assert torch.equal(layers._embed_rows(view, nodes, torch.bfloat16), view.index_select(0, nodes).to(torch.bfloat16))
    layer = _layer(64, False)
    assert not layers._embed_rows_kernel_ok(layer.embeds, nodes, torch.float64)
    with torch.no_grad():
        assert torch.equal(layer(nodes, dtype=torch.float64), layer.embeds.index_select(0, nodes).double())


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (1, 2, 4)), (torch.bfloat16, (1, 2, 4, 8))])
def test_gather_into_a_misaligned_view(dtype, offsets):
    """An ``out`` that starts off the row alignment (16 bytes for fp32 rows, 8 for bf16) is refused before the launch and keeps its
    bits; one that is aligned although it is a view into a larger buffer is served; nothing around it is written either way."""
    import het_amd.kernels as k
    from het_amd._lib import HetError
    K, B = 64, 65
    table, nodes = S.table(K).to(DEV), S.gather_ids(B).to(DEV)
    want = table.index_select(0, nodes).to(dtype)
    need = 16 if dtype == torch.float32 else 8
    for off in offsets:
        buf = torch.full((B * K + 2 * off,), 7.0, dtype=dtype, device=DEV)
        out = buf[off:off + B * K].view(B, K)
        if (out.data_ptr() % need) != 0:
            with pytest.raises(HetError, match="misaligned"):
                k.rows_embed_gather(table, nodes, dtype, out=out)
            torch.cuda.synchronize()
            assert bool((buf == 7.0).all()), off
        else:
            assert k.rows_embed_gather(table, nodes, dtype, out=out) is out
            assert torch.equal(out, want) and bool((buf[:off] == 7.0).all()) and bool((buf[off + B * K:] == 7.0).all()), off


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("K", (32, 64, 68))
@pytest.mark.parametrize("B", (0, 1, 65, 2049))
def test_sparse_backward(K, B):
    layer = _layer(K, True)
    nodes = S.gather_ids(B).to(DEV)
    go = torch.randn(B, K, generator=torch.Generator().manual_seed(B))
    for dtype, g in ((None, go), (torch.bfloat16, go.to(torch.bfloat16))):
        layer.embeds.grad = None
        out = layer(nodes, dtype=dtype)
        out.backward(g.to(DEV))
        grad = layer.embeds.grad
        assert grad.is_sparse and grad._nnz() == B and grad._values().dtype == torch.float32 and grad.shape == (S.N, K)
        assert torch.equal(grad._indices()[0], nodes)
        assert_close(grad.to_dense(), S.dense_ref(layer.embeds, ((nodes, g),))[1], what=f"sparse gradient, grad_out {g.dtype}")


@pytest.mark.parametrize("B", (0, 65, 2049))
def test_dense_backward_is_autograd_s_own(B):
    """sparse=False: the [N, K] gradient of forward(nodes) is, bit for bit, what embeds[nodes] gives (and for bf16 rows what
    embeds[nodes].to(bfloat16) gives)."""
    K = 64
    layer = _layer(K, False)
    nodes = S.gather_ids(B).to(DEV)
    go = torch.randn(B, K, generator=torch.Generator().manual_seed(B)).to(DEV)
    for dtype in (None, torch.bfloat16):
        g = go if dtype is None else go.to(dtype)
        layer.embeds.grad = None
        layer(nodes, dtype=dtype).backward(g)
        leaf = layer.embeds.detach().clone().requires_grad_(True)
        rows = leaf[nodes]
        (rows if dtype is None else rows.to(dtype)).backward(g)
        assert not layer.embeds.grad.is_sparse and torch.equal(layer.embeds.grad, leaf.grad)
        assert_close(layer.embeds.grad, S.dense_ref(layer.embeds, ((nodes, g),))[1])


@pytest.mark.parametrize("sparse", [False, True])
def test_autograd_contract_clauses(sparse):
    run_contract_clauses(lambda: _layer(64, sparse).cpu(), DEV)


# ------------------------------------------------------------------------------------------------ Adam
def _grads(pattern, B, K, steps=3):
    out = []
    for s in range(steps):
        ids, n, coalesced = S.adam_ids(pattern, B, s)
        out.append((ids, torch.randn(B, K, generator=torch.Generator().manual_seed(17 * s + B)), coalesced))
    return out, n


WORST = {}


@pytest.mark.parametrize("pattern", ("distinct", "one", "runs"))
@pytest.mark.parametrize("K", S.KS)
def test_adam_three_steps_on_the_ladder(K, pattern):
    """Three consecutive steps for every B of the ladder: d_hip <= 2 * d_ref + 2^-21 after each step (the pairs are printed)."""
    from het_amd.optim import RowSparseAdam
    worst = (0.0, 0.0)
    assert max(S.B_LADDER) > 2 * S.span(K)  # ("one": a run longer than a workgroup's span of positions)
    for B in S.B_LADDER:
        grads, n = _grads(pattern, B, K)
        if pattern == "runs" and B > S.span(K):
            assert all(S.runs_cross_spans(ids, K) for ids, _, _ in grads), "no run crosses a boundary between two workgroups' positions"
        worst = max(worst, S.three_steps(RowSparseAdam, DEV, K, grads, n=n, what=f"{pattern} B={B}"))
    WORST[(K, pattern)] = worst
    print(f"worst pair K={K} {pattern}: d_hip {worst[0]:.3e} d_ref {worst[1]:.3e}")


def _one_step(pattern, B, K, direct=False):
    """(p, m, v before, p, m, v after, ids, the leaf) of one step from preset non-zero moments."""
    from het_amd.optim import RowSparseAdam
    import het_amd.kernels as k
    ids, n, coalesced = S.adam_ids(pattern, B, 0)
    vals = torch.randn(B, K, generator=torch.Generator().manual_seed(B))
    p0, m0, v0 = S.start_state(n, K)
    p = p0.clone().to(DEV).requires_grad_(True)
    opt = S.make_optimizer(RowSparseAdam, p, m0, v0, **S.HYPER)
    st = opt.state[p]
    if direct:  # the kernel itself on sorted ids with perm = NULL (what a coalesced gradient with these rows would be, repeats kept)
        order = torch.sort(ids, stable=True).indices
        with torch.no_grad():
            k.rows_adam_(p, st["exp_avg"], st["exp_avg_sq"], ids[order].to(DEV), None, vals[order].contiguous().to(DEV), S.HYPER["lr"],
                         *S.HYPER["betas"], S.HYPER["eps"], 1)
    else:
        p.grad = S.sparse_grad(ids.to(DEV), vals.to(DEV), p.shape, coalesced)
        opt.step()
    torch.cuda.synchronize()
    return (p0, m0, v0), (p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()), ids, p


@pytest.mark.parametrize("pattern", ("distinct", "one", "runs"))
@pytest.mark.parametrize("K", S.KS)
def test_adam_leaves_other_rows_alone_and_repeats_its_bits(K, pattern):
    for B in (1, 65, 2049):
        before, after, ids, p = _one_step(pattern, B, K)
        untouched = torch.ones(before[0].shape[0], dtype=torch.bool)
        untouched[ids] = False
        assert bool(untouched.any()) and p._version >= 1
        for b, a, name in zip(before, after, ("p", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a[untouched], b[untouched]), f"{name}: a row outside the gradient changed (K={K} B={B} {pattern})"
            assert not torch.equal(a[ids], b[ids]), name
        again = _one_step(pattern, B, K)[1]
        for a, b in zip(after, again):
            assert torch.equal(a, b), "two identical runs differ in bits"
        # the same rows sorted by the caller and handed to the kernel with perm = NULL: the same sums in the same order
        direct = _one_step(pattern, B, K, direct=True)[1]
        for a, b in zip(after, direct):
            assert torch.equal(a, b), "perm = NULL on sorted rows differs from the sorted-by-the-optimizer step"


def test_adam_version_counter_and_saved_table():
    """The step writes p through a raw pointer: p._version rises, and a graph that saved the table refuses its stale copy."""
    from het_amd.optim import RowSparseAdam
    p = S.table(64).to(DEV).requires_grad_(True)
    opt = RowSparseAdam([p], **S.HYPER)
    loss = (p * p).sum()  # saves p
    v0 = p._version
    p.grad = S.sparse_grad(torch.tensor([3, 5, 3], device=DEV), torch.ones(3, 64, device=DEV), p.shape)
    opt.step()
    assert p._version == v0 + 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_adam_falls_back_off_the_kernel_s_shapes():
    """K = 10 on the GPU: the composed rule, the same bound."""
    from het_amd.optim import RowSparseAdam
    grads, n = _grads("runs", 257, 10)
    S.three_steps(RowSparseAdam, DEV, 10, grads, n=n, what="K=10 fallback")


# ------------------------------------------------------------------------------------------------ uninitialised memory
@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
def test_no_result_depends_on_uninitialised_memory(value):
    from het_amd.optim import RowSparseAdam

    def run():
        layer = _layer(64, True)
        opt = RowSparseAdam(layer.parameters(), **S.HYPER)
        nodes = S.gather_ids(257).to(DEV)
        go = torch.randn(257, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
        outs = []
        for dtype in (None, torch.bfloat16):
            out = layer(nodes, dtype=dtype)
            out.backward(go.to(out.dtype))
            opt.step()
            opt.zero_grad()
            outs.append(out.detach().clone())
        st = opt.state[layer.embeds]
        torch.cuda.synchronize()
        return outs + [layer.embeds.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]

    clean = run()
    with poisoned(value) as rec:
        dirty = run()
    assert rec.from_module("het_amd.kernels", "rows_embed_gather"), "the gather's output was not among the poisoned allocations"
    for a, b in zip(clean, dirty):
        assert bool(torch.isfinite(b.float()).all()) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ end to end
def test_train_sparse_embed_end_to_end(monkeypatch, capsys):
    """het_amd.train --sparse_embed runs, logs finite losses, and leaves every table row that no batch touched bit for bit at its
    seeded initial value -- dense Adam moves every row from the second step on."""
    from het_amd import layers, train
    seen = {}

    class Recording(layers.HET_RelGraphEmbed):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen["layer"], seen["init"], seen["nodes"] = self, self.embeds.detach().clone(), []

        def forward(self, nodes=None, dtype=None):
            seen["nodes"].append(nodes)
            return super().forward(nodes, dtype)

    monkeypatch.setattr(train, "HET_RelGraphEmbed", Recording)
    res = train.main(["--model", "rgcn", "--scale", "2e-3", "-e", "4", "--batch_size", "64", "--fanout", "5", "5", "--num_layers", "2",
                      "--sparse_embed"])
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"\| loss (\S+)", out)]
    assert len(losses) == 4 and all(math.isfinite(l) for l in losses) and math.isfinite(res["final_loss"])
    assert res["sparse_embed"] is True and res["args"]["sparse_embed"] is True
    layer = seen["layer"]
    assert layer.sparse and len(seen["nodes"]) == 9 and all(n is not None for n in seen["nodes"])  # 5 warm-up steps + 4 epochs
    # the seeded initial table, recomputed: main seeds torch, builds the graph, then the table
    torch.manual_seed(0)
    train.load_graph(train.argparse.Namespace(edges_npy=None, dataset="mag", scale=2e-3))
    again = layers.HET_RelGraphEmbed(layer.embeds.shape[0], 64).embeds.detach()
    assert torch.equal(again, seen["init"]), "the recorded initial table is not the seeded one"
    touched = torch.zeros(layer.embeds.shape[0], dtype=torch.bool)
    touched[torch.cat(seen["nodes"]).cpu()] = True
    final = layer.embeds.detach().cpu()
    assert bool(touched.any()) and bool((~touched).any()), "the batches touch no row, or every row: the check below would be empty"
    assert torch.equal(final[~touched], again[~touched]), "a row that no batch touched moved"
    assert bool((final[touched] != again[touched]).any()), "no touched row moved"
