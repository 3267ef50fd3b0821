"""Host logic of het_amd/plan.py: the per-thread override of the groupings switch and its propagation from an autograd
node's forward to its backward (no GPU, no library call)."""
import threading

import torch

import het_amd.plan as plan


def test_forced_is_per_thread_and_restores():
    assert plan.is_enabled() == plan.enabled
    seen = {}
    with plan.forced(False):
        assert plan.is_enabled() is False
        t = threading.Thread(target=lambda: seen.setdefault("other", plan.is_enabled()))
        t.start()
        t.join()
        with plan.forced(None):  # no override inside: the process-wide default again
            assert plan.is_enabled() == plan.enabled
        assert plan.is_enabled() is False
    assert seen["other"] == plan.enabled  # the other thread never saw the override
    assert plan.is_enabled() == plan.enabled


def test_backward_runs_with_the_choice_of_its_forward():
    seen = []

    @plan.consistent
    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            seen.append(("fwd", plan.is_enabled()))
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(("bwd", plan.is_enabled()))
            return g * 2

    x = torch.ones(3, requires_grad=True)
    with plan.forced(False):  # e.g. sampling.one_shot_graphs around the forward only
        y = Probe.apply(x)
    y.sum().backward()        # outside the block (and, on a GPU, on an autograd worker thread)
    z = Probe.apply(x)
    with plan.forced(False):
        z.sum().backward()    # a grouped forward keeps its grouped backward inside somebody else's one-shot block
    assert seen == [("fwd", False), ("bwd", False), ("fwd", plan.enabled), ("bwd", plan.enabled)]
    assert torch.equal(x.grad, torch.full((3,), 4.0))


# ---------------------------------------------------------------- inference tensors (no version counter) as cache sources
def test_ident_of_an_inference_tensor_does_not_raise():
    with torch.inference_mode():
        t = torch.arange(6)
    assert t.is_inference()
    assert plan._ident(t) == (t.data_ptr(), 6, plan.NO_VERSION)
    assert plan._ident(None) is None
    n = torch.arange(6)
    assert plan._ident(n) == (n.data_ptr(), 6, n._version) and n._version >= 0
    assert plan.cacheable(plan._ident(n), None) and not plan.cacheable(plan._ident(n), plan._ident(t))


def test_what_a_cache_builds_is_a_normal_tensor_in_any_mode():
    import het_amd.kernels as k
    src = torch.arange(5)  # built outside: a normal tensor, as a graph made before the evaluation loop
    with torch.inference_mode():
        assert (src * 2).is_inference()  # (what the builder would return without plan.building)
        built = k._derived_get("test_plan_doubled", (src,), lambda: src * 2)
        with plan.building():
            kept = torch.empty(3)
    assert not built.is_inference() and not kept.is_inference() and not built.requires_grad
    assert k._derived_get("test_plan_doubled", (src,), lambda: 1 / 0) is built  # cached: the builder is not asked again

    class Save(torch.autograd.Function):  # a training step afterwards saves it for its backward: torch accepts it
        @staticmethod
        def forward(ctx, x, idx):
            ctx.save_for_backward(idx)
            return x[idx]

        @staticmethod
        def backward(ctx, g):
            return torch.zeros(20).index_add_(0, ctx.saved_tensors[0], g), None

    x = torch.ones(20, requires_grad=True)
    Save.apply(x, built).sum().backward()
    assert float(x.grad.sum()) == 5.0


def test_an_inference_source_is_never_served_a_stale_entry():
    """An inference tensor's in-place edit moves no version counter: a lookup with such a source builds every time and keeps
    nothing; a normal source hits until its version moves."""
    import het_amd.kernels as k
    calls = []

    def doubled(t):
        return k._derived_get("test_plan_stale", (t,), lambda: (calls.append(1), t * 2)[1])

    with torch.inference_mode():
        t = torch.arange(4)
        first = doubled(t)
        t.copy_(torch.tensor([7, 5, 3, 1]))  # e.g. the eids renumbered in place
        second = doubled(t)
        assert not first.is_inference() and not second.is_inference()
    assert first.tolist() == [0, 2, 4, 6] and second.tolist() == [14, 10, 6, 2] and len(calls) == 2
    assert not any(key[0] == "test_plan_stale" for key in k._derived)  # nothing was kept
    n = torch.arange(4)
    a, b = doubled(n), doubled(n)
    assert a is b and len(calls) == 3
    n.copy_(torch.tensor([7, 5, 3, 1]))
    assert doubled(n).tolist() == [14, 10, 6, 2] and len(calls) == 4


def test_a_graph_made_in_inference_mode_is_refused_where_a_gradient_is_needed():
    """... by every layer at its entry (a HetError that says why), on the CPU as on the GPU: nothing has been launched by then;
    a graph made outside is not refused, whatever mode its lazily built lists are first needed in."""
    import pytest

    from het_amd._lib import HetError
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel, HET_HGTLayerHetero, HET_RGATLayer
    from het_amd.synth import make_random
    outside = HetGraph.from_integrated_coo(make_random(40, 3, 200, seed=1), full=False)
    with torch.inference_mode():
        inside = HetGraph.from_integrated_coo(make_random(40, 3, 200, seed=1))
        outside.generate_separate_unique_node_indices_single_sided_for_each_etype()
        outside.get_in_csr()
        st, _ = outside.get_rel_node_types()
    assert inside.holds_inference_tensors() and not outside.holds_inference_tensors() and not st.is_inference()
    x = torch.randn(40, 16, requires_grad=True)
    calls = [(HET_RGATLayer(16, 16, 3, 2, dropout=0.0), (x,)),
             (HET_EglRelGraphConv_EdgeParallel(16, 16, 3), (x, torch.rand(200, 1))),
             (HET_HGTLayerHetero(1, 3, 16, 16, num_heads=2), (x,))]
    for layer, args in calls:
        with pytest.raises(HetError, match="created in inference mode"):
            layer(inside, *args)
    for p in calls[0][0].parameters():
        p.requires_grad_(False)
    assert calls[0][0]._route(inside, x.detach(), None, False).path == "composition"  # nothing needs a gradient: routed, not refused


def test_a_sampler_made_in_inference_mode_samples_outside_it():
    """Its scratch map is written in place by every sample_block: a normal tensor whatever mode the sampler was made in."""
    from het_amd.graph import HetGraph
    from het_amd.sampling import NeighborSampler
    from het_amd.synth import make_random
    g = HetGraph.from_integrated_coo(make_random(40, 3, 200, seed=1))
    with torch.inference_mode():
        sampler = NeighborSampler(g, [-1])
    assert not sampler._map.is_inference()
    b = sampler.sample_block(torch.arange(10), -1)
    assert b.num_dst == 10 and not b.graph.holds_inference_tensors()
