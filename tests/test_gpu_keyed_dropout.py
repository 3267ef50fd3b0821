"""Keyed dropout on the GPU (csrc/keyed_dropout.hip, het_amd/layers.py KeyedDropout): the kernels against the numpy rule of
tests/_keyed_dropout_ref.py bit for bit (same_bits: torch.equal on the bit patterns, a NaN equal to a NaN), the autograd node, what
it keeps for the backward, and the RGAT / RGCN layers with ``keyed_dropout=True`` against the same layers without dropout."""
import functools
import hashlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _keyed_dropout_ref as ref
from tests._keyed_dropout_ref import same_bits
from tests._poison import POISON_IDS, POISONS, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, DRAW = 12345, 3
# The kernels run a grid-stride loop over at most 2048 workgroups of 256 lanes, one group of 4 elements per lane and iteration
# (csrc/keyed_dropout.hip: kDropMaxBlocks): from LOOP_N elements on, lanes take a second group, and the last group is a tail of 1.
LOOP_N = 2048 * 256 * 4 + 5
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097 * 100, LOOP_N)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _input(n, dtype, seed):
    """(CPU tensor, its copy on the GPU) of tests/_keyed_dropout_ref.special_input: made once, shared, never written."""
    t = ref.special_input(n, dtype, seed)
    return t, t.to(DEV)


def _check(n, dtype, relu, p, base=0, alias=False):
    import het_amd.kernels as k
    (y, yd), (go, god) = _input(n, dtype, 1), _input(n, dtype, 2)
    out = k.keyed_dropout(yd, p, SEED, DRAW, relu=relu, base=base)
    want = ref.forward(y, p, SEED, DRAW, relu, base)
    same_bits(out, want, f"out n={n}")
    want_g = ref.backward(go, want, p, SEED, DRAW, relu, base)
    if alias:
        buf = god.clone()
        gy = k.keyed_dropout_backward(buf, out if relu else None, p, SEED, DRAW, relu=relu, base=base, grad_y=buf)
        assert gy.data_ptr() == buf.data_ptr()
    else:
        gy = k.keyed_dropout_backward(god, out if relu else None, p, SEED, DRAW, relu=relu, base=base)
    same_bits(gy, want_g, f"grad_y n={n}")
    # what the calls read is what it was
    same_bits(yd, y, "y after the calls")
    same_bits(god, go, "grad_out after the calls")
    same_bits(out, want, "out after the backward")
    return out, gy


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 65535.0 / 65536.0], ids=["p0", "p0.1", "p0.5", "pmax"])
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_kernels_are_the_rule_bit_for_bit(dtype, relu, p):
    for n in SIZES:
        _check(n, DTYPES[dtype], relu, p)


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_base_above_2_to_the_32nd_groups(dtype):
    for n in (9, 4097):
        _check(n, DTYPES[dtype], True, 0.5, base=1 << 40)
    assert not np.array_equal(ref.mask(SEED, DRAW, 1 << 40, 4097, 0.5), ref.mask(SEED, DRAW, 0, 4097, 0.5))


@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_grad_y_may_be_grad_out(dtype, relu):
    for n in (7, 1025, 4097 * 100):
        _check(n, DTYPES[dtype], relu, 0.5, alias=True)


@pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_every_element_is_written(dtype, value):
    """Under a poison in everything the wrappers allocate, the same bits come out: no element of out or grad_y is left unwritten."""
    for n in (5, 1025, 4097 * 100):
        with poisoned(value) as rec:
            _check(n, DTYPES[dtype], True, 0.5)
        assert len(rec.from_module("het_amd.kernels")) >= 2, rec  # (out and grad_y were poisoned)


# ---------------------------------------------------------------- the autograd node
def _module(p=0.5, act="relu"):
    from het_amd.layers import KeyedDropout
    return KeyedDropout(p, act, seed=SEED)


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_node_takes_expanded_and_strided_grad_out(dtype):
    dt = DTYPES[dtype]
    y = _input(64 * 33, dt, 1)[0].view(33, 64)
    yd = y.to(DEV).requires_grad_(True)
    m = _module()
    out = m(yd, draw=DRAW)
    want = ref.forward(y, 0.5, SEED, DRAW, True)
    same_bits(out, want, "out")
    gx, = torch.autograd.grad(out.sum(), yd, retain_graph=True)  # an expanded (stride-0) grad_out
    same_bits(gx, ref.backward(torch.ones_like(y), want, 0.5, SEED, DRAW, True), "expanded grad_out")
    go_t = _input(64 * 33, dt, 2)[1].view(64, 33)
    gx, = torch.autograd.grad(out.t(), yd, go_t, retain_graph=True)  # the node sees go_t.t(): a column-strided grad_out
    want_g = ref.backward(go_t.t().cpu().contiguous(), want, 0.5, SEED, DRAW, True)
    same_bits(gx, want_g, "strided grad_out")
    gx2, = torch.autograd.grad(out.t(), yd, go_t)  # the graph walked a second time
    same_bits(gx2, gx, "second walk")


def test_node_launches_nothing_for_an_input_without_gradient(monkeypatch):
    import het_amd.kernels as k
    from het_amd.layers import _KeyedDropoutFunction
    m = _module()
    y = torch.randn(40, 64, device=DEV)
    out = m(y, draw=DRAW)
    assert not out.requires_grad and out.grad_fn is None
    monkeypatch.setattr(k, "keyed_dropout_backward", lambda *a, **kw: pytest.fail("a backward launch for an input that needs no gradient"))
    ctx = types.SimpleNamespace(needs_input_grad=(False,) * 6, key=(0.5, SEED, DRAW, 0, True), saved_tensors=(out,))
    assert _KeyedDropoutFunction.backward(ctx, torch.ones_like(out)) == (None,) * 6


def test_eval_under_inference_mode_is_the_activation_alone():
    y = torch.randn(40, 64, device=DEV)
    m = _module().eval()
    with torch.inference_mode():
        assert torch.equal(m(y), torch.relu(y)) and m.draw == 0
        assert _module(act=None).eval()(y) is y
    m.train()
    with torch.inference_mode():  # training mode without autograd: the kernel's forward, nothing kept
        same_bits(m(y, draw=DRAW), ref.forward(y.cpu(), 0.5, SEED, DRAW, True), "inference-mode training call")


def test_what_the_node_keeps():
    packed = []
    y = torch.randn(1 << 22, device=DEV, requires_grad=True)  # 16 MiB of out: the allocator's 512-byte rounding is far below 1 %
    for act, floats in (("relu", 1), (None, 0)):
        m = _module(act=act)
        del packed[:]
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (packed.append(t), t)[1], lambda t: t):
            out = m(y)
        grew = torch.cuda.memory_allocated() - before
        kept = [t for t in packed if t.is_floating_point()]
        assert len(kept) == floats, [tuple(t.shape) for t in kept]
        assert all(t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr() for t in kept)  # out itself, no copy
        nbytes = out.numel() * out.element_size()
        print(f"{act}: memory_allocated grew by {grew} bytes for {nbytes} bytes of out")
        assert nbytes <= grew <= 1.01 * nbytes
        del out


# ---------------------------------------------------------------- the layers
H_EXCLUDE = 1e-4  # two runs of a layer differ in the last bits where float atomics sum: the sign of an h this close to zero is open


def _layer_case(kind, dtype, keyed=True):
    """(graph, keyed layer or None, plain layer -- no activation, no dropout -- with the same parameters, x, norm or None, oracle h in
    fp64) on tests.util.ladder_graph."""
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel, HET_RGATLayer
    from oracle import layers as OL
    from tests.util import ladder_graph
    torch.manual_seed(11)
    g = ladder_graph(R=5, seed=5, shuffle=False)
    N, E, R, K, X = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels(), 64, 64
    s = g.get_separate_coo_original()
    kw = dict(self_loop=True, bf16_training=dtype == torch.bfloat16) if kind == "rgat" else {}
    make = (lambda **o: HET_RGATLayer(K, X, R, 4, **kw, **o)) if kind == "rgat" else (lambda **o: HET_EglRelGraphConv_EdgeParallel(K, X, R, **o))
    plain = make(activation=None, dropout=0.0)
    with torch.no_grad():  # a bias away from zero: a node without in-edges has h = bias (RGCN), which must not sit at the kink of relu
        plain.h_bias.copy_((torch.rand(X) * 0.05 + 0.05) * (torch.randint(0, 2, (X,)) * 2 - 1))
    x = (torch.randn(N, K) * 0.5).to(dtype)
    norm = torch.rand(E, 1) if kind == "rgcn" else None
    p = {n: t.detach().double() for n, t in plain.named_parameters()}
    if kind == "rgat":
        h = OL.rgat_layer(x.double(), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, 0.2,
                          p["loop_weight"], p["h_bias"])
    else:
        h = OL.rgcn_layer(x.double(), p["weight"], norm.double()[s["eids"]], s["rel_ptrs"], s["row_indices"], s["col_indices"], N, p["h_bias"])
    layer = None
    if keyed:
        layer = make(activation=F.relu, dropout=0.5, keyed_dropout=True)
        layer.load_state_dict(plain.state_dict())
    return g, layer, plain, x, norm, h


def _close(name, got, want, dtype):
    from tests._bf16_rows_ref import check_bf16
    from tests.util import assert_close
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.dtype == torch.bfloat16:
        check_bf16(name, got, want.float())
    else:
        assert_close(got, want, what=name)


@pytest.mark.parametrize("kind,dtype,block", [("rgat", "fp32", False), ("rgat", "fp32", True), ("rgat", "bf16", False), ("rgat", "bf16", True),
                                              ("rgcn", "fp32", False), ("rgcn", "bf16", False)])
def test_layers_with_keyed_dropout(kind, dtype, block):
    dt = DTYPES[dtype]
    g, keyed, plain, x, norm, h64 = _layer_case(kind, dt)
    nd = 1000 if block else g.get_num_nodes()
    share64 = float((h64[:nd].abs() < H_EXCLUDE).double().mean())
    assert share64 <= 0.01, share64  # the oracle's h: almost nothing sits at the kink
    g.to_(DEV)
    keyed, plain = keyed.to(DEV).train(), plain.to(DEV).train()
    extra = () if norm is None else (norm.to(DEV),)
    kw = dict(num_dst=nd) if block else {}
    xp, xk = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    h = plain(g, xp, *extra, **kw)
    out = keyed(g, xk, *extra, **kw)
    assert out.shape == h.shape == (nd, 64) and out.dtype == dt and keyed.dropout.draw == 1
    seed, scale = keyed.dropout.seed, ref.params(0.5)[1]
    kept = torch.from_numpy(ref.mask(seed, 0, 0, out.numel(), 0.5)).view(out.shape).to(DEV)
    dropped = out.detach()[~kept]
    assert bool((dropped == 0).all()) and not bool(torch.signbit(dropped).any())  # exactly +0 where the reference drops
    assert 0.45 < float((~kept).double().mean()) < 0.55
    want = torch.relu(h.detach().float()) * float(scale)
    _close("kept outputs", torch.where(kept, out.detach(), torch.zeros_like(out)), torch.where(kept, want, torch.zeros_like(want)), dt)
    near = h.detach().float().abs() < H_EXCLUDE
    share = float(near.double().mean())
    print(f"{kind} {dtype}: |h| < {H_EXCLUDE:g} on {share:.4%} of the elements (oracle: {share64:.4%})")
    assert share <= 0.01
    go = torch.randn(nd, 64).to(dt).to(DEV).masked_fill(near, 0)
    out.backward(go)
    h.backward(ref.backward(go, out.detach(), 0.5, seed, 0, relu=True).to(DEV))  # the rule's backward as the plain layer's cotangent
    g.cpu_()
    _close("grad_x", xk.grad, xp.grad, dt)
    for (name, a), (_, b) in zip(keyed.named_parameters(), plain.named_parameters()):
        assert a.grad is not None and b.grad is not None, name
        _close("grad " + name, a.grad, b.grad, dt)


def default_layer_drop_pattern(kind):
    """sha256 of where a default (keyed_dropout=False) layer with relu and dropout 0.5, in training, for torch.manual_seed(1234), has
    zeros in its output -- among the elements whose oracle |h| exceeds 1e-3, where the sign of h does not depend on the order float
    atomics summed in: there the zeros are relu's (h < 0, from the oracle) and nn.Dropout's (the torch generator's)."""
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel, HET_RGATLayer
    g, _, plain, x, norm, h64 = _layer_case(kind, torch.float32, keyed=False)
    if kind == "rgat":
        layer = HET_RGATLayer(64, 64, 5, 4, activation=F.relu, dropout=0.5, self_loop=True)
    else:
        layer = HET_EglRelGraphConv_EdgeParallel(64, 64, 5, activation=F.relu, dropout=0.5)
    layer.load_state_dict(plain.state_dict())
    g.to_(DEV)
    layer = layer.to(DEV).train()
    extra = () if norm is None else (norm.to(DEV),)
    torch.manual_seed(1234)
    out = layer(g, x.to(DEV), *extra).detach().cpu()
    g.cpu_()
    sel = h64.abs() > 1e-3
    assert float(sel.double().mean()) > 0.95
    zeros = (out == 0)[sel]
    assert bool(zeros[(h64 < 0)[sel]].all())  # relu's zeros are there
    share = float(zeros[(h64 > 0)[sel]].double().mean())
    assert 0.45 < share < 0.55, share  # and about half of the rest: dropout ran
    return hashlib.sha256(np.packbits(zeros.numpy()).tobytes()).hexdigest()


# recorded from a run of the parent commit (the tree before keyed dropout existed) on an MI355X
PARENT_DROP_PATTERN = {
    "rgat": "709422b95eb10736dff3f7b0a60e14f648136d05a72c5cb901c12dde836c5e8c",
    "rgcn": "eb08e173546907c82e90bff975bdc32a7e3eb527e3c2f815a6fcf3ed879cc5a2",
}


@pytest.mark.parametrize("kind", ["rgat", "rgcn"])
def test_default_layers_drop_what_they_dropped(kind):
    """keyed_dropout=False changes nothing: for a fixed torch seed the default layer zeroes the elements it zeroed before."""
    assert default_layer_drop_pattern(kind) == PARENT_DROP_PATTERN[kind]
