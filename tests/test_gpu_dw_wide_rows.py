"""The wide-row instance of the 64 x 64 fp32 weight gradient (csrc/seg_gemm_mfma.hip: HET_seg_dw_mfma_wide -- 16-byte row loads
feeding v_mfma_f32_16x16x4_f32) against fp64 products of the same rows, at the row counts where its row groups of 4, its clamped
tail, its waves without rows, its 512-row chunks and its two-batch loop can go wrong; and the instance it replaces on the calls
that must keep it (rows on 8-byte boundaries, HET_DW_WIDE_ROWS=0).  Which instance ran is read from the library's per-kernel
timer labels.  Tolerance: tests/util.assert_close, what tests/test_gpu_ops.py holds rows_matmul_backward_dw / matmul_backward to."""
import pytest
import torch

from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = X = 64
ROWS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 511, 512, 513, 1025)
LAYOUTS = {"R1": None,                      # one relation of n rows (n from ROWS)
           "R3_empty_middle": (513, 0, 7),
           "R4_unequal": (1, 1025, 5, 33)}
LISTS = ("identity", "gather_a", "gather_both")


def _launches(fn):
    """(launches of the wide instance, launches of either instance) while fn() runs."""
    from het_amd import _lib
    _lib.kernel_timing(True)
    try:
        fn()
        wide = _lib.kernel_timing_read("HET_seg_dw_mfma<wide>")[1]
        both = _lib.kernel_timing_read("HET_seg_dw_mfma")[1]
    finally:
        _lib.kernel_timing(False)
    return wide, both


def _rows(n_rows, width, seed):
    """Rows whose magnitudes differ (x1 ... x5 by row, the last row the largest): a row entering twice or not at all moves the sums
    by far more than the tolerance."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(n_rows, width, generator=gen)
    mag = 1.0 + (torch.arange(n_rows) % 4).float()
    if n_rows:
        mag[-1] = 5.0
    return t * mag.view(-1, 1)


def _case(sizes, lists, seed):
    """Segment pointers, the two row tensors and the two row lists (None = identity) of one call."""
    n = sum(sizes)
    rp = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0).tolist()), dtype=torch.int64)
    gen = torch.Generator().manual_seed(seed + 1)
    na = n if lists == "identity" else n // 2 + 3          # fewer table rows than positions: duplicate ids, out of order
    ng = n if lists != "gather_both" else n // 3 + 2
    a, g = _rows(na, K, seed + 2), _rows(ng, X, seed + 3)
    ia = None if lists == "identity" else torch.randint(0, na, (n,), generator=gen)
    ig = None if lists != "gather_both" else torch.randint(0, ng, (n,), generator=gen)
    return rp, a, g, ia, ig


def _reference(rp, a, g, ia, ig, H):
    """fp64: dW[r] = A[ia]^T . G[ig] per relation as [R, H, K, D], and the column sums of the G rows of the call."""
    n = int(rp[-1])
    ar = (a[:n] if ia is None else a[ia]).double()
    gr = (g[:n] if ig is None else g[ig]).double()
    D = X // H
    dw = torch.stack([(ar[int(rp[r]):int(rp[r + 1])].t() @ gr[int(rp[r]):int(rp[r + 1])]).view(K, H, D).permute(1, 0, 2)
                      for r in range(rp.numel() - 1)])
    return dw, gr.sum(0)


def _dw(rp, a, g, ia, ig, grad_w, accumulate, colsum=None):
    """The C entry itself: the Python wrapper takes no row list for gradout."""
    import het_amd.kernels as k
    from het_amd import _lib
    R, H, _, D = grad_w.shape
    p = k._p
    if colsum is None:
        _lib.call("het_rows_matmul_backward_dw", p(rp), R, p(ia), p(ig), int(rp[-1]), p(a), p(g), p(grad_w), H, K, D, int(accumulate),
                  k._stream(g))
    else:
        _lib.call("het_rows_matmul_backward_dw_colsum", p(rp), R, p(ia), p(ig), int(rp[-1]), p(a), p(g), p(grad_w), p(colsum), H, K, D,
                  int(accumulate), k._stream(g))


def _check(sizes, lists, H, seed):
    rp, a, g, ia, ig = _case(sizes, lists, seed)
    dw_ref, cs_ref = _reference(rp, a, g, ia, ig, H)
    rpd, ad, gd = rp.to(DEV), a.to(DEV), g.to(DEV)
    iad, igd = (None if t is None else t.to(DEV) for t in (ia, ig))
    R, D = len(sizes), X // H
    # "=" with column sums (both outputs start from values that must not survive)
    gw, cs = torch.full((R, H, K, D), 7.0, device=DEV), torch.full((X,), 7.0, device=DEV)
    wide, both = _launches(lambda: _dw(rpd, ad, gd, iad, igd, gw, False, cs))
    assert (wide, both) == (1, 1), f"the wide-row instance was not chosen ({wide} of {both} launches)"
    assert_close(gw, dw_ref, what="grad_w (=, column sums)")
    assert_close(cs, cs_ref, what="colsum")
    # "+=" onto a non-zero gradient, no column sums
    base = torch.randn(R, H, K, D, generator=torch.Generator().manual_seed(seed + 4))
    gw2 = base.to(DEV)
    wide, both = _launches(lambda: _dw(rpd, ad, gd, iad, igd, gw2, True))
    assert (wide, both) == (1, 1), f"the wide-row instance was not chosen ({wide} of {both} launches)"
    assert_close(gw2, base.double() + dw_ref, what="grad_w (+=)")


@pytest.mark.parametrize("lists", LISTS)
@pytest.mark.parametrize("n", ROWS)
def test_rows_per_relation(n, lists):
    """One relation of n rows into the layer's [R, H, K, D] layout: the row group of 4, the clamped tail and waves without rows
    (n < 16), the 512-row chunk (511, 512, 513: one and two workgroups) and the two-batch loop boundary; column sums with a
    partial last batch."""
    _check((n,), lists, 4, 100 + n)


@pytest.mark.parametrize("lists", LISTS)
@pytest.mark.parametrize("H", [4, 1], ids=["headcat_4_heads", "headcat_1_head"])
@pytest.mark.parametrize("layout", ["R3_empty_middle", "R4_unequal"])
def test_relation_layouts(layout, H, lists):
    """Several relations per launch (an empty one in the middle; very unequal sizes), into the head-concatenated layout with four
    heads, [R, 4, 64, 16], and with one, [R, 1, 64, 64] (the same bytes as the plain layout, but still the head-concatenated branch
    of the kernel: the plain one is test_plain_layout)."""
    _check(LAYOUTS[layout], lists, H, 7 + len(layout))


def test_plain_layout():
    """The plain [K][X] output layout (headcat == 0), which only the RGCN layer's backward asks for: its weight gradient
    grad_w[r] = ssum[(r, v)]^T . gradout[v] over the (relation, destination) rows -- row i of `A`, a row list on `G` -- at
    K = D = 64, without the input gradient, so that the weight gradient is the entry's one matrix-core launch."""
    import het_amd.kernels as k
    from tests.util import random_graph
    g = random_graph(seed=91, n=500, r=4, e=6000, shuffle=False)  # (relation 1 is empty)
    s = g.get_separate_coo_original()
    N, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    gen = torch.Generator().manual_seed(92)
    x, go = _rows(N, K, 93), _rows(N, X, 94)
    w, norm = torch.randn(R, K, X, generator=gen) * 0.1, torch.rand(E, generator=gen) + 0.5
    rel = torch.repeat_interleave(torch.arange(R), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    msg = (norm[s["eids"]].view(-1, 1) * x[s["row_indices"]]).double()  # the norm is indexed by edge id
    gdst = go[s["col_indices"]].double()
    ref = torch.stack([msg[rel == r].t() @ gdst[rel == r] for r in range(R)])
    g.to_(DEV)
    sd = g.get_separate_coo_original()
    plan = k.rgcn_layer_plan(sd["rel_ptrs"], sd["eids"], sd["row_indices"], sd["col_indices"], N)
    assert plan is not None
    normd = norm.to(DEV)
    _, ssum = k.rgcn_layer_forward(plan, x.to(DEV), w.to(DEV), normd, None)
    out = {}
    wide, both = _launches(lambda: out.update(gw=k.rgcn_layer_backward(plan, ssum, w.transpose(1, 2).contiguous().to(DEV), normd,
                                                                       go.to(DEV), want_bias=False, want_x=False)[1]))
    g.cpu_()
    assert (wide, both) == (1, 1), f"the wide-row instance was not chosen ({wide} of {both} launches)"
    assert_close(out["gw"], ref, what="grad_w [R, K, X]")


def _kind1_backward(x, go, idx, rp, H, Kh, D, in1head):
    """matmul_backward on a unique (relation, node) list (kind 1: no grouping, gradout row i): (grad_w, grad_x)."""
    import het_amd.kernels as k
    R, N = rp.numel() - 1, x.shape[0]
    d = {"unique_srcs_and_dests_rel_ptrs": rp, "unique_srcs_and_dests_node_indices": idx}
    wt = torch.randn(R, H, D, Kh, generator=torch.Generator().manual_seed(5)).to(DEV)
    gx = torch.empty(N, Kh if in1head else H * Kh, device=DEV)
    gw = torch.full((R, H, Kh, D), 7.0, device=DEV)
    k.matmul_backward(d, 1, wt, x, go, gx, gw, in1head, accumulate=False)
    return gw


def test_block_diagonal_layout():
    """The third output layout: per-head 16 x 16 blocks of the 64 x 64 product (a2's backward with a per-head input), the rest of
    the product dropped."""
    H, Kh, D, sizes = 4, 16, 16, (37, 0, 514)
    n, N = sum(sizes), 300
    rp = torch.tensor([0, 37, 37, 551], dtype=torch.int64)
    gen = torch.Generator().manual_seed(21)
    idx = torch.randint(0, N, (n,), generator=gen)
    x, go = _rows(N, H * Kh, 22), _rows(n, H * D, 23)
    out = {}
    wide, both = _launches(lambda: out.update(gw=_kind1_backward(x.to(DEV), go.to(DEV), idx.to(DEV), rp.to(DEV), H, Kh, D, False)))
    assert (wide, both) == (1, 1), f"the wide-row instance was not chosen ({wide} of {both} launches)"
    xs, g64 = x[idx].double().view(n, H, Kh), go.double().view(n, H, D)
    for r in range(3):
        a, b = int(rp[r]), int(rp[r + 1])
        assert_close(out["gw"][r], torch.einsum("nhk,nhd->hkd", xs[a:b], g64[a:b]), what=f"grad_w[{r}]")


def _offset8(t):
    """A copy of t that starts 8 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[2:2 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


@pytest.mark.parametrize("n", [5, 513, 1025])
def test_rows_on_8_byte_boundaries_keep_the_old_instance(n):
    """The same call with x offset by 8 bytes runs HET_seg_dw_mfma<2, 2> (its float-pair loads need 8-byte alignment only) and
    gives the same result within the tolerance.  gradout offset by 8 bytes: no entry point hands such rows to either matrix-core
    instance (a2's backward takes them to the any-shape kernels), so the call must simply not reach the wide one."""
    H, D, N = 4, 16, n // 2 + 3
    rp = torch.tensor([0, n // 3, n], dtype=torch.int64)
    gen = torch.Generator().manual_seed(31 + n)
    idx = torch.randint(0, N, (n,), generator=gen)
    x, go = _rows(N, K, 32 + n), _rows(n, X, 33 + n)
    xs = x[idx].double()
    ref = torch.stack([(xs[int(rp[r]):int(rp[r + 1])].t() @ go[int(rp[r]):int(rp[r + 1])].double()).view(K, H, D).permute(1, 0, 2)
                       for r in range(2)])
    xd, god, idxd, rpd = x.to(DEV), go.to(DEV), idx.to(DEV), rp.to(DEV)
    for what, xa, ga, expect in (("aligned", xd, god, (1, 1)), ("x + 8 bytes", _offset8(xd), god, (0, 1)),
                                 ("gradout + 8 bytes", xd, _offset8(god), (0, 0))):
        out = {}
        got = _launches(lambda: out.update(gw=_kind1_backward(xa, ga, idxd, rpd, H, K, D, True)))
        assert got == expect, f"{what}: (wide, either) launches {got}, expected {expect}"
        assert_close(out["gw"], ref, what=f"grad_w, {what}")


def _switch_case(expect):
    """The three row-list forms of one call (column sums included): which instance ran, and the result against fp64."""
    sizes, H = (9, 1025, 0, 30), 4
    for lists in LISTS:
        rp, a, g, ia, ig = _case(sizes, lists, 57)
        dw_ref, cs_ref = _reference(rp, a, g, ia, ig, H)
        rpd, ad, gd = rp.to(DEV), a.to(DEV), g.to(DEV)
        iad, igd = (None if t is None else t.to(DEV) for t in (ia, ig))
        gw, cs = torch.full((len(sizes), H, K, X // H), 7.0, device=DEV), torch.full((X,), 7.0, device=DEV)
        got = _launches(lambda: _dw(rpd, ad, gd, iad, igd, gw, False, cs))
        assert got == expect, f"{lists}: (wide, either) launches {got}, expected {expect}"
        assert_close(gw, dw_ref, what=f"grad_w, {lists}")
        assert_close(cs, cs_ref, what=f"colsum, {lists}")


def test_switch_forces_the_old_instance():
    """HET_DW_WIDE_ROWS=0 (read once per process, hence a fresh child): the calls that take the wide instance here run
    HET_seg_dw_mfma<2, 2> there, with the same result within the tolerance -- column sums included."""
    import os
    import subprocess
    import sys
    _switch_case((1, 1))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import tests.test_gpu_dw_wide_rows as t; t._switch_case((0, 1)); print('SWITCH_OK')"
    env = dict(os.environ, HET_DW_WIDE_ROWS="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SWITCH_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
