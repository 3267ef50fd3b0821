"""tests/_autograd_contract.py on the CPU: an honest stand-in layer passes every clause, and one planted defect per clause is caught
by that clause.  The stand-in is a small torch.autograd.Function -- out[dst] += (x @ W)[src] over a toy edge list, plus a bias -- with
an fp64 oracle; the defects are variations of it in pure torch.  None of them is in the library and none runs on a GPU.

Which clauses catch which defect is asserted as a whole matrix: every defect by its own clause and by no other, with one overlap that
follows from the clauses' definitions -- C1 watches ``go`` too, so the defect of C2 (a backward that writes into a contiguous
incoming gradient, which in C1 is the caller's ``go`` itself) is caught by both."""
import functools

import pytest
import torch

from tests import _autograd_contract as AC
from tests.util import assert_close

N, K, X, E = 23, 6, 5, 60
CLAUSES = sorted(AC.CLAUSES)


class ToyGraph:
    def __init__(self):
        gen = torch.Generator().manual_seed(11)
        self.src = torch.randint(0, N, (E,), generator=gen)
        self.dst = torch.randint(0, N - 3, (E,), generator=gen)  # (the last nodes receive nothing)

    def to_(self, dev):
        self.src, self.dst = self.src.to(dev), self.dst.to(dev)
        return self


# module-level state of the defects (reset by every make())
STATE = {}


class Honest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        xc = x.contiguous()
        ctx.save_for_backward(xc, W, src, dst)
        return torch.zeros(x.shape[0], W.shape[1], dtype=x.dtype).index_add_(0, dst, (xc @ W)[src]) + b

    @staticmethod
    def backward(ctx, g):
        x, W, src, dst = ctx.saved_tensors
        g = g.contiguous()
        gm = torch.zeros(x.shape[0], W.shape[1], dtype=g.dtype).index_add_(0, src, g[dst])  # gradient of x @ W
        need = ctx.needs_input_grad
        return (gm @ W.t() if need[0] else None), (x.t() @ gm if need[1] else None), (g.sum(0) if need[2] else None), None, None


class WritesX(Honest):
    """C1: the forward writes into x through .data (one unit in the last place: no value test notices)."""
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        x.data[0, 0] = torch.nextafter(x.data[0, 0], torch.tensor(float("inf"), dtype=x.dtype))
        return Honest.forward(ctx, x, W, b, src, dst)


class ScalesIncomingGradient(Honest):
    """C2: the backward scales the incoming gradient in place (where ``.contiguous()`` hands it the caller's tensor) and compensates."""
    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        g.mul_(2.0)
        return tuple(None if t is None else 0.5 * t for t in Honest.backward(ctx, g))


class AssumesContiguousGradient(Honest):
    """C3: the backward reads grad.view(-1), which assumes contiguity."""
    @staticmethod
    def backward(ctx, g):
        return Honest.backward(ctx, g.view(-1).view(g.shape))


class NoInputGradMeansNoGrad(Honest):
    """C4: ``not x.requires_grad`` is treated as "nothing requires a gradient"."""
    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return Honest.backward(ctx, g)


class ZeroesSavedTensor(Honest):
    """C5: the backward zeroes a saved tensor through .data after using it (a buffer "given back")."""
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        xs = x.detach().clone()  # (a copy: x itself stays as it was, C1 holds)
        ctx.save_for_backward(xs, W, src, dst)
        return torch.zeros(x.shape[0], W.shape[1], dtype=x.dtype).index_add_(0, dst, (xs @ W)[src]) + b

    @staticmethod
    def backward(ctx, g):
        grads = Honest.backward(ctx, g)
        ctx.saved_tensors[0].data.zero_()
        return grads


class ReturnsViewOfSharedBuffer(Honest):
    """C6: the forward of a training call returns a view of a module-level buffer, which the backward retires."""
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        out = Honest.forward(ctx, x, W, b, src, dst)
        if STATE.get("out") is None or STATE["out"].shape != out.shape or STATE["out"].dtype != out.dtype:
            with torch.inference_mode(False):  # (a normal tensor in any mode: the defect is the sharing, nothing else)
                STATE["out"] = torch.empty_like(out)
        STATE["out"].copy_(out)
        return STATE["out"].view_as(out)

    @staticmethod
    def backward(ctx, g):
        STATE["out"] = None
        return Honest.backward(ctx, g)


class ReturnsSharedWeightGradient(Honest):
    """C7: the backward returns a module-level buffer as the weight gradient -- one buffer per call that is alive at the same time
    (a pool indexed by the number of forwards whose backward has not run), so two calls in one graph do not collide, but the next
    step is handed the buffer the previous step's gradient was returned in."""
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        ctx.slot = STATE["live"] = STATE.get("live", -1) + 1
        return Honest.forward(ctx, x, W, b, src, dst)

    @staticmethod
    def backward(ctx, g):
        gx, gw, gb, _, _ = Honest.backward(ctx, g)
        STATE["live"] -= 1
        if gw is not None:
            if STATE.get(("gw", ctx.slot)) is None:
                STATE["gw", ctx.slot] = torch.empty_like(gw)
            gw = STATE["gw", ctx.slot].copy_(gw)
        return gx, gw, gb, None, None


class CachesIndexOnFirstUse(Honest):
    """C8: an index tensor is cached on first use -- inside torch.inference_mode() an inference tensor -- and saved for backward."""
    @staticmethod
    def forward(ctx, x, W, b, src, dst):
        if STATE.get("src64") is None:
            STATE["src64"] = src + 0
        return Honest.forward(ctx, x, W, b, STATE["src64"], dst)


FUNCTIONS = {"honest": Honest, "C1": WritesX, "C2": ScalesIncomingGradient, "C3": AssumesContiguousGradient, "C4": NoInputGradMeansNoGrad,
             "C5": ZeroesSavedTensor, "C6": ReturnsViewOfSharedBuffer, "C7": ReturnsSharedWeightGradient, "C8": CachesIndexOnFirstUse}


class ToyLayer(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.fn = fn
        self.weight = torch.nn.Parameter(torch.randn(K, X, generator=gen) * 0.4)
        self.bias = torch.nn.Parameter(torch.randn(X, generator=gen) * 0.1)

    def forward(self, g, x):
        return self.fn.apply(x, self.weight, self.bias, g.src, g.dst)


@functools.lru_cache(maxsize=None)
def _inputs(seed, block=False):
    gen = torch.Generator().manual_seed(100 + seed)
    return torch.randn(N, K, generator=gen) * 0.5, torch.randn(N, X, generator=gen)


_ORACLE = {}


def _oracle(calls):
    key = AC.fingerprint(*(t for x, go, _ in calls for t in (x, go)))
    if key not in _ORACLE:
        ref, g = ToyLayer(Honest), ToyGraph()
        W, b = ref.weight.detach().double().requires_grad_(True), ref.bias.detach().double().requires_grad_(True)
        xs = [x.double().requires_grad_(True) for x, _, _ in calls]
        outs = [torch.zeros(N, X, dtype=torch.float64).index_add(0, g.dst, (x @ W)[g.src]) + b for x in xs]
        grads = torch.autograd.grad(sum((o * go.double()).sum() for o, (_, go, _) in zip(outs, calls)), xs + [W, b])
        _ORACLE[key] = AC.Expected([o.detach() for o in outs], list(grads[:len(xs)]), {"weight": grads[-2], "bias": grads[-1]})
    return _ORACLE[key]


def _case(which):
    def make():
        STATE.clear()
        layer, graph = ToyLayer(FUNCTIONS[which]), ToyGraph()

        def call(x, block=False):
            return layer(graph, x)
        call.block_graph = None
        call.operands = lambda: {"src": graph.src, "dst": graph.dst}
        return layer, graph, call
    return AC.Case(name=which, make=make, leaves=("weight", "bias"), inputs=_inputs, oracle=_oracle,
                   close=lambda a, e, what: assert_close(a, e, what=what), frozen=("bias",))


@pytest.mark.parametrize("clause", CLAUSES)
def test_the_honest_stand_in_passes(clause):
    AC.run_clause(clause, _case("honest"), "cpu")


# (the defect of C2 writes into the caller's contiguous ``go``: C1 watches that tensor too)
CAUGHT_BY = {c: {c} for c in CLAUSES}
CAUGHT_BY["C2"] = {"C1", "C2"}


@pytest.mark.parametrize("clause", CLAUSES)
@pytest.mark.parametrize("defect", CLAUSES)
def test_a_planted_defect_is_caught_by_its_clause_and_no_other(defect, clause):
    case = _case(defect)
    if clause not in CAUGHT_BY[defect]:
        AC.run_clause(clause, case, "cpu")
    elif clause == "C8":  # torch's own refusal surfaces as it is
        with pytest.raises(RuntimeError, match="Inference tensors cannot be saved for backward"):
            AC.run_clause(clause, case, "cpu")
    else:
        with pytest.raises(AssertionError, match=clause):
            AC.run_clause(clause, case, "cpu")


def test_the_strided_forms_are_not_contiguous_and_hold_the_values():
    x, go = _inputs(1)
    for name, make in AC._x_forms(x).items():
        v = AC._rebuild(make, _case("honest"), "cpu")
        assert not v.is_contiguous() and torch.equal(v, x), name
    for name, (make, values) in AC._go_forms(go).items():
        v = AC._rebuild(make, _case("honest"), "cpu")
        assert not v.is_contiguous() and torch.equal(v, values), name
    assert AC._rebuild(AC._go_forms(go)["expanded"][0], _case("honest"), "cpu").stride() == (0, 1)
