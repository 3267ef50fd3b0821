"""What torch.autograd may do with a layer, as clauses that any layer can be held to ("The autograd contract").

The parity tests call a layer the same way every time: one forward, one ``out.backward(go)`` with a fresh contiguous ``go``, every
leaf requiring a gradient, nothing else alive.  A training script hands over gradients that are strided or shared, walks a graph
twice, keeps two calls of one layer alive, freezes leaves, slices its input and evaluates under ``torch.inference_mode()`` before it
trains.  Each clause below is one such pattern, written once as a function of a ``Case`` and a device; tests/test_gpu_autograd_
contract.py runs them on every autograd node of the layers, tests/test_autograd_contract_harness.py on a CPU stand-in and on one
planted defect per clause.

Bit-equality (``torch.equal``) is asked only where nobody may write: operands, outputs returned earlier, the gradient of a residual
branch.  Everything computed is held to the case's fp64 oracle through ``Case.close``, because float atomics make two runs differ.

No GPU import here: a device is an argument."""
import dataclasses
import hashlib
from typing import Callable, Dict, Optional, Tuple

import torch


@dataclasses.dataclass
class Expected:
    """The oracle's answer for one or several calls made in one autograd graph: the output and the input gradient of every call,
    and per leaf name the gradient summed over the calls."""
    outs: list
    gx: list
    gp: Dict[str, object]


@dataclasses.dataclass
class Case:
    """One layer configuration.
    make()                     -> (layer, graph, call), all on the CPU, the graph built outside any grad mode.  ``layer`` is an
                                  nn.Module (``named_parameters`` are the leaves); ``graph`` has ``to_(device)``; ``call(x)`` ->
                                  out, ``call(x, block=True)`` the same layer on ``call.block_graph`` (moved with the graph).
                                  ``call.operands()`` -> name -> tensor: what C1 watches beside x, go and the parameters (RGCN's norm,
                                  the index tensors of the graph's separate COO), asked after the move to the device.
    leaves                     the parameter names
    inputs(seed, block=False)  -> (x, go): fp32 CPU tensors (values the case's dtype holds exactly), for the graph or the block
    oracle(calls)              calls = ((x, go, block), ...) made in one autograd graph -> Expected, in fp64
    close(actual, expected, what)   raises AssertionError when ``actual`` is not ``expected`` within the case's tolerance
    dtype                      of x, go and the output on the device
    frozen                     the leaves C4 (c) freezes (attention / relation-prior parameters; RGCN: the bias)
    block                      the layer takes num_dst: the block half of C6 runs"""
    name: str
    make: Callable
    leaves: Tuple[str, ...]
    inputs: Callable
    oracle: Callable
    close: Callable
    dtype: torch.dtype = torch.float32
    frozen: Tuple[str, ...] = ()
    block: bool = False


def fingerprint(*tensors):
    """A key for caching oracle results by the VALUES (and layout) of their inputs."""
    h = hashlib.sha1()
    for t in tensors:
        h.update(repr((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- helpers
def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _setup(case, dev, frozen=()):
    layer, graph, call = case.make()
    layer.to(dev)
    graph.to_(dev)
    if getattr(call, "block_graph", None) is not None:
        call.block_graph.to_(dev)
    call.operands()  # (whatever the case moves to the device with its operands is moved now, outside every grad mode)
    for n, p in layer.named_parameters():
        p.requires_grad_(n not in frozen)
        p.grad = None
    return layer, graph, call


def _on(case, t, dev):
    """A fresh contiguous copy of a CPU tensor on the device in the case's dtype (never the cached tensor itself)."""
    return t.detach().clone().to(dev).to(case.dtype)


def _leaf(case, t, dev, grad=True):
    return _on(case, t, dev).requires_grad_(grad)


def _params(layer):
    return dict(layer.named_parameters())


def _check_grads(case, layer, exp, what, frozen=()):
    """The gradient of every leaf that is not frozen is the oracle's; a frozen leaf has none."""
    params = _params(layer)
    assert set(params) == set(case.leaves), f"{what}: the layer's parameters {sorted(params)} are not the case's leaves"
    for n in case.leaves:
        if n in frozen:
            assert params[n].grad is None, f"{what}: the frozen leaf {n} received a gradient"
        else:
            assert params[n].grad is not None, f"{what}: the leaf {n} received no gradient"
            case.close(params[n].grad, exp.gp[n], f"{what} grad_{n}")


def _check_x(case, actual, expected, like, what):
    assert actual is not None, f"{what}: no gradient"
    assert actual.shape == like.shape and actual.dtype == like.dtype, f"{what}: {tuple(actual.shape)} {actual.dtype} for an input {tuple(like.shape)} {like.dtype}"
    case.close(actual, expected, what)


def _zero(layer, *leaves):
    for p in layer.parameters():
        p.grad = None
    for t in leaves:
        t.grad = None


# ---------------------------------------------------------------- C1
def c1_operands_untouched(case, dev):
    """After forward, backward and a synchronize, x, go, every parameter and every operand the case names are bit for bit what they
    were."""
    layer, graph, call = _setup(case, dev)
    x, go = case.inputs(1)
    xd, god = _leaf(case, x, dev), _on(case, go, dev)
    watch = {"x": xd, "go": god, **_params(layer), **call.operands()}
    before = {k: v.detach().clone() for k, v in watch.items()}
    out = call(xd)
    out.backward(god)
    _sync(dev)
    for k, v in watch.items():
        assert torch.equal(v.detach(), before[k]), f"C1 {case.name}: the operand {k} was written during the step"
    exp = case.oracle(((x, go, False),))
    case.close(out, exp.outs[0], f"C1 {case.name} out")


# ---------------------------------------------------------------- C2
def c2_shared_gradient(case, dev):
    """(layer(x) + skip).backward(go): both branches receive the same tensor.  skip.grad is go bit for bit, go is unchanged; x also
    feeds (x * w_in).sum(), and x.grad is the oracle's gradient + w_in -- a returned grad_x may be added into in place.
    A bf16 x is the cast of an fp32 leaf here (so that autograd adds the two terms in fp32, not in bf16 with a second rounding that no
    bf16 bound of the project covers), and the known term w_in is taken off again before the layer's term meets its bound: the fp32
    add and the fp64 subtract leave 2^-24 |w_in| <= 2e-8, rounding that back to bf16 returns the layer's bf16 value."""
    layer, graph, call = _setup(case, dev)
    x, go = case.inputs(1)
    gen = torch.Generator().manual_seed(202)
    w_in = (0.25 * torch.randn(x.shape, generator=gen)).to(case.dtype).float()
    skip = _leaf(case, torch.randn(go.shape, generator=gen), dev)
    god, wd = _on(case, go, dev), w_in.to(dev)
    keep = god.clone()
    if case.dtype == torch.float32:
        leaf = xin = _leaf(case, x, dev)
    else:
        leaf = x.detach().clone().to(dev).requires_grad_(True)  # fp32
        xin = leaf.to(case.dtype)
    out = call(xin)
    side = (leaf * wd).sum()
    torch.autograd.backward([out + skip, side], [god, torch.ones((), device=dev)])
    _sync(dev)
    assert torch.equal(god, keep), f"C2 {case.name}: the gradient handed to two branches was written"
    assert skip.grad is not None and torch.equal(skip.grad, keep), f"C2 {case.name}: the residual branch did not receive go bit for bit"
    exp = case.oracle(((x, go, False),))
    if case.dtype == torch.float32:
        _check_x(case, leaf.grad, exp.gx[0] + w_in.double(), leaf, f"C2 {case.name} grad_x (+ w_in)")
    else:
        got = (leaf.grad.double() - wd.double()).to(case.dtype)
        case.close(got, exp.gx[0], f"C2 {case.name} grad_x (w_in taken off)")
    _check_grads(case, layer, exp, f"C2 {case.name}")


# ---------------------------------------------------------------- C3
def _x_forms(x):
    """(a) a column slice of a wider tensor, (b) the transpose of a [K, N] tensor: the values of x, no row contiguous with the next."""
    N, K = x.shape
    wide = torch.full((N, K + 8), 7.0)
    wide[:, 4:4 + K] = x
    return {"column_slice": lambda t=wide: t[:, 4:4 + K], "transposed": lambda t=x.t().contiguous(): t.t()}


def _go_forms(go):
    """(a) one row expanded, stride (0, 1); (b) transposed storage; (c) a column slice.  Returns name -> (make view, its values)."""
    n, X = go.shape
    row = go[:1].clone()
    wide = torch.full((n, X + 8), 7.0)
    wide[:, 4:4 + X] = go
    return {"expanded": (lambda t=row: t.expand(n, X), row.expand(n, X).contiguous()),
            "transposed": (lambda t=go.t().contiguous(): t.t(), go),
            "column_slice": (lambda t=wide: t[:, 4:4 + X], go)}


C3_FORMS = (("column_slice", "expanded"), ("transposed", "transposed"), ("column_slice", "column_slice"), ("transposed", "expanded"))


def c3_strides(case, dev, x_form, go_form):
    """x and go as non-contiguous views (``x_form`` of _x_forms, ``go_form`` of _go_forms), built on the device from storage in the
    case's dtype: output and all gradients are the oracle's, x.grad has x's shape.  A layer that raises on such an operand has
    broken the clause as much as one that computes from the wrong memory."""
    layer, graph, call = _setup(case, dev)
    x, go = case.inputs(1)
    go_view, go_values = _go_forms(go)[go_form]
    base_x = _x_forms(x)[x_form]
    # the views are taken ON the device, of device storage in the case's dtype (a .to() of a view would make it contiguous)
    xd = _rebuild(base_x, case, dev).requires_grad_(True)
    god = _rebuild(go_view, case, dev)
    assert not xd.is_contiguous() and not god.is_contiguous() and xd.is_leaf
    try:
        out = call(xd)
        out.backward(god)
        _sync(dev)
    except RuntimeError as e:
        raise AssertionError(f"C3 {case.name}: the layer raised on x {x_form} / go {go_form}: {e}") from e
    exp = case.oracle(((x, go_values, False),))
    what = f"C3 {case.name} x {x_form} go {go_form}"
    case.close(out, exp.outs[0], what + " out")
    _check_x(case, xd.grad, exp.gx[0], xd, what + " grad_x")
    _check_grads(case, layer, exp, what)


def _rebuild(make_view, case, dev):
    """The view ``make_view`` takes of a CPU tensor, taken of a copy of that tensor's storage on the device in the case's dtype."""
    view = make_view()
    base = view._base if view._base is not None else view
    root = base.detach().clone().to(dev).to(case.dtype)
    return torch.as_strided(root, view.shape, view.stride(), view.storage_offset())


# ---------------------------------------------------------------- C4
def c4_frozen_leaves(case, dev, sub):
    """sub "a": x without a gradient, every parameter with one; "b": every parameter frozen, x with one; "c": the case's ``frozen``
    leaves frozen; "d": nothing requires a gradient with grad mode on -- out.requires_grad is False and out is the oracle's.
    In a - c the remaining gradients are the oracle's and the frozen leaves have none."""
    frozen = {"a": (), "b": case.leaves, "c": case.frozen, "d": case.leaves}[sub]
    x_grad = sub in ("b", "c")
    layer, graph, call = _setup(case, dev, frozen)
    x, go = case.inputs(1)
    xd, god = _leaf(case, x, dev, x_grad), _on(case, go, dev)
    assert torch.is_grad_enabled()
    out = call(xd)
    exp = case.oracle(((x, go, False),))
    what = f"C4({sub}) {case.name}"
    case.close(out, exp.outs[0], what + " out")
    if sub == "d":
        assert not out.requires_grad, f"{what}: nothing requires a gradient, the output does"
        return
    assert out.requires_grad, f"{what}: the output requires no gradient"
    out.backward(god)
    _sync(dev)
    if x_grad:
        _check_x(case, xd.grad, exp.gx[0], xd, what + " grad_x")
    else:
        assert xd.grad is None, f"{what}: an input that requires no gradient received one"
    _check_grads(case, layer, exp, what, frozen)


# ---------------------------------------------------------------- C5
def c5_second_backward(case, dev):
    """out.backward(go1, retain_graph=True) gives the oracle's gradients for go1; after clearing them, out.backward(go2) through the
    same node gives the oracle's for go2."""
    layer, graph, call = _setup(case, dev)
    x, go1 = case.inputs(1)
    _, go2 = case.inputs(2)
    xd = _leaf(case, x, dev)
    out = call(xd)
    for i, (go, retain) in enumerate(((go1, True), (go2, False))):
        _zero(layer, xd)
        out.backward(_on(case, go, dev), retain_graph=retain)
        _sync(dev)
        exp = case.oracle(((x, go, False),))
        what = f"C5 {case.name} backward {i + 1}"
        _check_x(case, xd.grad, exp.gx[0], xd, what + " grad_x")
        _check_grads(case, layer, exp, what)


# ---------------------------------------------------------------- C6
def c6_interleaved_calls(case, dev, block=False):
    """oa = layer(g, xa); ob = layer(g, xb) (``block``: on the sampled block) before either backward; one backward of
    (oa * ga).sum() + (ob * gb).sum().  oa keeps its bits through the second forward and the backward; both input gradients and the
    parameter gradients (both calls in one graph) are the oracle's."""
    layer, graph, call = _setup(case, dev)
    xa, ga = case.inputs(1)
    xb, gb = case.inputs(2, block) if block else case.inputs(2)
    xad, xbd = _leaf(case, xa, dev), _leaf(case, xb, dev)
    oa = call(xad)
    _sync(dev)
    keep = oa.detach().clone()
    ob = call(xbd, block=True) if block else call(xbd)
    _sync(dev)
    what = f"C6 {case.name}{' (block)' if block else ''}"
    assert torch.equal(oa.detach(), keep), f"{what}: the first output changed when the layer was called again"
    ((oa * _on(case, ga, dev)).sum() + (ob * _on(case, gb, dev)).sum()).backward()
    _sync(dev)
    assert torch.equal(oa.detach(), keep), f"{what}: the first output changed during the backward"
    exp = case.oracle(((xa, ga, False), (xb, gb, block)))
    case.close(oa, exp.outs[0], what + " out a")
    case.close(ob, exp.outs[1], what + " out b")
    _check_x(case, xad.grad, exp.gx[0], xad, what + " grad_xa")
    _check_x(case, xbd.grad, exp.gx[1], xbd, what + " grad_xb")
    _check_grads(case, layer, exp, what)


# ---------------------------------------------------------------- C7
def c7_returned_tensors_are_owned(case, dev):
    """out1 and grads1 (torch.autograd.grad: the tensors the node returned, not copies) keep their bits through a whole second step
    on other inputs; and two backward calls without zeroing leave .grad = g1 + g2.
    A bf16 x.grad would be a bf16 sum of two bf16 terms (a second rounding, under cancellation outside every bf16 bound of the
    project): there x is the cast of an fp32 leaf, and each term meets its own bound -- .grad after the first call, and the difference
    the second call made (an fp32 add: 2^-24 relative, far inside the absolute term of those bounds)."""
    layer, graph, call = _setup(case, dev)
    x1, go1 = case.inputs(1)
    x2, go2 = case.inputs(2)
    names = list(case.leaves)
    params = _params(layer)
    x1d = _leaf(case, x1, dev)
    out1 = call(x1d)
    grads1 = torch.autograd.grad(out1, [x1d] + [params[n] for n in names], _on(case, go1, dev))
    _sync(dev)
    keep = [t.detach().clone() for t in (out1,) + tuple(grads1)]
    x2d = _leaf(case, x2, dev)
    out2 = call(x2d)
    grads2 = torch.autograd.grad(out2, [x2d] + [params[n] for n in names], _on(case, go2, dev))
    _sync(dev)
    for n, t, k in zip(["out"] + ["grad_x"] + ["grad_" + n for n in names], (out1,) + tuple(grads1), keep):
        assert torch.equal(t.detach(), k), f"C7 {case.name}: {n} of the first step changed during the second"
    e1, e2 = case.oracle(((x1, go1, False),)), case.oracle(((x2, go2, False),))
    for exp, out, grads, step in ((e1, out1, grads1, 1), (e2, out2, grads2, 2)):
        case.close(out, exp.outs[0], f"C7 {case.name} step {step} out")
        case.close(grads[0], exp.gx[0], f"C7 {case.name} step {step} grad_x")
        for n, g in zip(names, grads[1:]):
            case.close(g, exp.gp[n], f"C7 {case.name} step {step} grad_{n}")
    del out1, out2, grads1, grads2
    # two backward calls, nothing zeroed in between
    e12 = case.oracle(((x1, go2, False),))
    _zero(layer)
    if case.dtype == torch.float32:
        leaf = _leaf(case, x1, dev)
        feed = lambda: leaf
    else:
        leaf = x1.detach().clone().to(dev).requires_grad_(True)
        feed = lambda: leaf.to(case.dtype)
    call(feed()).backward(_on(case, go1, dev))
    _sync(dev)
    first = leaf.grad.detach().clone()
    call(feed()).backward(_on(case, go2, dev))
    _sync(dev)
    what = f"C7 {case.name} two backward calls"
    if case.dtype == torch.float32:
        _check_x(case, leaf.grad, e1.gx[0] + e12.gx[0], leaf, what + " grad_x")
    else:
        case.close(first.to(case.dtype), e1.gx[0], what + " grad_x, first term")
        case.close((leaf.grad.double() - first.double()).to(case.dtype), e12.gx[0], what + " grad_x, second term")
    for n in names:
        case.close(params[n].grad, e1.gp[n] + e12.gp[n], f"{what} grad_{n}")


# ---------------------------------------------------------------- C8 (I1)
GRAD_MODES = {"inference_mode": torch.inference_mode, "no_grad": torch.no_grad}


def c8_evaluate_then_train(case, dev, mode="inference_mode"):
    """I1: the graph is built outside; the first call ever on it runs inside ``mode`` with x created inside the block, and is the
    oracle's; a training step on the same graph and layer afterwards is the oracle's in output and every gradient.  A layer that
    caches what it builds on first use as it comes (an inference tensor) and later saves it for a backward meets torch's own error
    here ("Inference tensors cannot be saved for backward"): that error is the finding, it is not converted."""
    layer, graph, call = _setup(case, dev)
    x, go = case.inputs(1)
    with GRAD_MODES[mode]():
        xe = _on(case, x, dev)  # created inside: an inference tensor under inference_mode
        out = call(xe)
        _sync(dev)
    assert not out.requires_grad
    exp = case.oracle(((x, go, False),))
    case.close(out, exp.outs[0], f"C8 {case.name} out under {mode}")
    xd = _leaf(case, x, dev)
    out = call(xd)
    out.backward(_on(case, go, dev))
    _sync(dev)
    what = f"C8 {case.name} training step after {mode}"
    case.close(out, exp.outs[0], what + " out")
    _check_x(case, xd.grad, exp.gx[0], xd, what + " grad_x")
    _check_grads(case, layer, exp, what)


CLAUSES = {"C1": c1_operands_untouched, "C2": c2_shared_gradient, "C3": c3_strides, "C4": c4_frozen_leaves, "C5": c5_second_backward,
           "C6": c6_interleaved_calls, "C7": c7_returned_tensors_are_owned, "C8": c8_evaluate_then_train}


def run_clause(name, case, dev):
    """Clause ``name`` with every parameter value it has (the forms of C3, the sub-cases of C4, both halves of C6, both modes of C8)."""
    f = CLAUSES[name]
    if name == "C3":
        for xf, gf in C3_FORMS:
            f(case, dev, xf, gf)
    elif name == "C4":
        for sub in "abcd":
            f(case, dev, sub)
    elif name == "C6":
        f(case, dev)
        if case.block:
            f(case, dev, True)
    elif name == "C8":
        for mode in GRAD_MODES:
            f(case, dev, mode)
    else:
        f(case, dev)
