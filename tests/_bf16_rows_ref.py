"""References and checkers of tests/test_gpu_bf16_ladders.py that need no GPU: the operations behind the bf16 row entries as plain
torch compositions in the dtype of their arguments -- fp64 for the reference, fp32 for the measurement of the absolute term of the bf16
bound and for the "results" tests/test_bf16_rows_ref.py feeds the checkers --, and the checkers themselves, which the GPU tests and
that CPU file share.

Rules of every case: bf16 inputs are drawn in fp32 and rounded once, the reference is evaluated on the
rounded values (exact inputs), and nothing rounds inside these operations but the single store of a bf16 output.
  fp32 outputs (sums, ret, run sums, every gradient): tests/util.py::assert_close at its defaults, the bound of the fp32 twins.
  bf16 outputs: elementwise |out - ref| <= 2^-8 |ref| + a max|ref| (tests/test_gpu_rgcn_bf16.py::_check_bf16); a = ABS_TERM."""
import torch

from tests.util import ROW_LADDER, assert_close, row_ladder_ptrs

BF16 = torch.bfloat16
REL = 2.0 ** -8  # twice the half-ulp of bf16: the rounding of the store, and one more for a sum that lands beside a rounding boundary
# The absolute term a: measure_abs_term() over every case of tests/test_bf16_rows_ref.py -- the smallest a for which the fp32 CPU
# evaluation of the reference, rounded to bf16, passes against the fp64 one -- gives 0 .. 2.8e-7 (an fp32 sum that cancels to
# nearly nothing beside a rounding boundary; the largest: h_inout, 4 heads of 32, the hub graph); times 4, the project's margin for the GPU's other summation order (tests/test_gpu_rgat_bf16.py), that stays below
# the 1e-5 of tests/test_gpu_rgcn_bf16.py::_check_bf16, which is the floor.  tests/test_bf16_rows_ref.py prints the per-case values
# and asserts 4 a <= ABS_TERM.  Never taken from a HIP result.
ABS_FLOOR = 1e-5
ABS_TERM = 1e-5


def bf16_round(t):
    return t.to(BF16).to(t.dtype)


def bf16_input(*shape, gen, scale=1.0):
    """A bf16 input: drawn in fp32, rounded once."""
    return (torch.randn(*shape, generator=gen) * scale).to(BF16)


def smallest_abs_term(out, ref):
    """The smallest a for which every element of ``out`` satisfies |out - ref| <= 2^-8 |ref| + a max|ref|."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return max(0.0, float(((out - ref).abs() - REL * ref.abs()).max() / ref.abs().max().clamp_min(1e-300)))


def measure_abs_term(ref64, ref32):
    """The absolute term one bf16 output needs: the fp32 evaluation, rounded once to bf16 (what a correct kernel stores, in one of the
    possible summation orders), against the fp64 evaluation."""
    return smallest_abs_term(ref32.to(BF16), ref64)


# ---- checkers -------------------------------------------------------------------------------------------------------------------
def check_bf16(name, out, ref, a=ABS_TERM):
    """A bf16 output rounded once from an fp32 sum of exact products against its fp64 reference, elementwise."""
    assert out.dtype == BF16, f"{name}: {out.dtype}"
    assert tuple(out.shape) == tuple(ref.shape), f"{name}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    o, r = out.detach().double().cpu(), ref.detach().double().cpu()
    if r.numel() == 0:
        return
    assert bool(torch.isfinite(o).all()), f"{name}: {int((~torch.isfinite(o)).sum())} elements are not finite"
    d = (o - r).abs()
    bound = REL * r.abs() + a * float(r.abs().max())
    worst = float((d - bound).max())
    print(f"{name}: max excess over 2^-8 |ref| + {a:g} max|ref| {worst:.2e}")
    assert worst <= 0, f"{name}: {int((d > bound).sum())} elements outside 2^-8 |ref| + {a:g} max|ref| (worst excess {worst:.2e})"


def check_f32(name, out, ref):
    """An fp32 output against its fp64 reference: the bound of the fp32 twins (tests/util.py::assert_close at its defaults)."""
    assert out.dtype == torch.float32, f"{name}: {out.dtype}"
    assert tuple(out.shape) == tuple(ref.shape), f"{name}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    assert_close(out, ref, what=name)


def check_per_relation(name, out, ref, rel_ptrs):
    """check_f32 relation by relation (a weight gradient [R, ...]), the row count of the relation in the message."""
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape), f"{name}: {out.dtype} {tuple(out.shape)}"
    for r in range(ref.shape[0]):
        check_f32(f"{name}[{r}] ({int(rel_ptrs[r + 1] - rel_ptrs[r])} rows)", out[r], ref[r])


def check_same_bits(name, out, before, rows):
    """The rows ``rows`` (bool [n] or index list) of ``out`` hold the bits of ``before``: the entry did not write them."""
    a, b = out.detach().cpu()[rows], before.detach().cpu()[rows]
    same = torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF16 else torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same, f"{name}: rows the entry must not write were written"


def check_aggregate(name, got, ref, a=ABS_TERM):
    """The outputs of rgat_aggregate_compact_bf16 against rgat_runs_reference (or the oracle's values in the same layout).
    got: sum [N,H], ret [N,H,D], q_rows [S_col,H,D], q_sum / q_ref [S_col,H] fp32, h_inout [N,X] bf16 (the whole tensor the entry was
    given the first nh rows of), h_before (its bits before the call).  ref: lse, ret, q_sum, q_rows (the run sums on the scale of
    exp(s), not relative to a maximum), has_in [N] bool, nh, h_ref [nh,X] (= h0 + ret)."""
    has_in, nh = ref["has_in"], ref["nh"]
    N = has_in.numel()
    sm = got["sum"].detach().cpu()
    check_f32(f"{name} log-sum-exp", sm[has_in], ref["lse"][has_in])
    assert float(sm[~has_in].abs().max() if bool((~has_in).any()) else 0.0) == 0.0, f"{name}: log-sum-exp of a destination without in-edges"
    check_f32(f"{name} ret", got["ret"].detach().cpu()[has_in], ref["ret"][has_in])
    sc = torch.exp(got["q_ref"].detach().double().cpu())  # the run sums are relative to q_ref: back to the scale of exp(s)
    assert got["q_sum"].dtype == torch.float32 and got["q_rows"].dtype == torch.float32
    assert_close(got["q_sum"].detach().double().cpu() * sc, ref["q_sum"], what=f"{name} q_sum")
    assert_close(got["q_rows"].detach().double().cpu() * sc.unsqueeze(-1), ref["q_rows"], what=f"{name} q_rows")
    wrote = has_in.clone()
    wrote[nh:] = False
    h = got["h_inout"].detach().cpu()
    assert h.shape[0] == N
    check_bf16(f"{name} h_inout", h[:nh][wrote[:nh]], ref["h_ref"][wrote[:nh]], a)
    check_same_bits(f"{name} h_inout (no in-edges, or beyond h_rows)", h, got["h_before"], ~wrote)


def check_backward(name, got, ref):
    """The gradients of rgat_backward_compact_bf16 (all fp32) against rgat_runs_reference: grad_feat, grad_el, grad_er and, where
    given, grad_bias and grad_attn_l."""
    for key in ("grad_feat", "grad_el", "grad_er", "grad_bias", "grad_attn_l"):
        assert (got.get(key) is None) == (ref.get(key) is None), f"{name}: {key}"
        if got.get(key) is not None:
            check_f32(f"{name} {key}", got[key], ref[key])


def check_node_dx(name, grad_x, ref, zero_rows, a=ABS_TERM):
    """grad_x of rgat_node_backward_dx_bf16: the elementwise bf16 bound, and exact zeros for the nodes no term reaches."""
    check_bf16(name, grad_x, ref, a)
    z = grad_x.detach().cpu()[zero_rows]
    assert float(z.float().abs().max() if z.numel() else 0.0) == 0.0, f"{name}: a node without any term is not exactly zero"


# ---- dense row operations, in the dtype of their arguments -------------------------------------------------------------------------
def rel_of_rows(rel_ptrs):
    R = rel_ptrs.numel() - 1
    return torch.repeat_interleave(torch.arange(R), rel_ptrs[1:] - rel_ptrs[:-1])


def rows_matmul(rel_ptrs, xs, W):
    """y[i] = xs[i] . W[r(i)]: xs [n,K] (already gathered), W [R,K,X]."""
    out = torch.zeros(xs.shape[0], W.shape[2], dtype=xs.dtype)
    for r in range(W.shape[0]):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        out[a:b] = xs[a:b] @ W[r]
    return out


def heads_to_columns(W):
    """[R,H,K,D] (the RGAT layer's head-concatenated weight) as [R,K,H*D]."""
    R, H, K, D = W.shape
    return W.permute(0, 2, 1, 3).reshape(R, K, H * D)


def rows_matmul_dw(rel_ptrs, xs, gs, R):
    """grad_w[r] = SUM over the rows i of relation r of xs[i]^T (x) gs[i]: [R,K,X]."""
    out = torch.zeros(R, xs.shape[1], gs.shape[1], dtype=xs.dtype)
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        out[r] = xs[a:b].t() @ gs[a:b]
    return out


def rows_dot1h(rel_ptrs, xs, w):
    """out[i,h] = <xs[i], w[r(i),h]>: w [R,H,K]."""
    out = torch.zeros(xs.shape[0], w.shape[1], dtype=xs.dtype)
    for r in range(w.shape[0]):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        out[a:b] = xs[a:b] @ w[r].t()
    return out


def rows_dot1h_dw(rel_ptrs, xs, go, R):
    """grad_w[r,h] = SUM_i gradout[i,h] * xs[i] over the rows of relation r: [R,H,K]."""
    return rows_matmul_dw(rel_ptrs, go, xs, R)


def el_rows(rel_ptrs, feat, attn):
    """el[u,h] = <feat[u,h,:], attn[r(u),h,:]>."""
    return (feat * attn[rel_of_rows(rel_ptrs)]).sum(-1)


def node_rows_sum(N, sources):
    """out[n] = SUM_s rows_s[map_s[n]] . wt_s; sources: (rows, map [N] long with -1 = none, or None = the node id, wt [KS,XO])."""
    out = torch.zeros(N, sources[0][2].shape[1], dtype=sources[0][0].dtype)
    for rows, m, wt in sources:
        if m is None:
            n = min(N, rows.shape[0])
            out[:n] += rows[:n] @ wt
        else:
            has = m >= 0
            out[has] += rows[m[has]] @ wt
    return out


def node_dx(N, n_loop, gh, loop_w, g_rows, W, rp_row, n_row, g_er, wa, rp_col, n_col):
    """grad_x of the node-major pass (include/het_amd.h: het_rgat_node_backward_dx) term by term: gh [n_loop,X] or None, loop_w [K,X],
    g_rows [S_row,X], W [R,H,K,D], g_er [S_col,H] or None, wa [R,H,K]."""
    R, H, Kd, D = W.shape
    gx = torch.zeros(N, Kd, dtype=g_rows.dtype)
    if gh is not None:
        gx[:n_loop] += gh[:n_loop] @ loop_w.t()
    for r in range(R):
        a, b = int(rp_row[r]), int(rp_row[r + 1])
        gx.index_add_(0, n_row[a:b], g_rows[a:b] @ W[r].permute(1, 0, 2).reshape(Kd, H * D).t())
        if g_er is not None:
            a, b = int(rp_col[r]), int(rp_col[r + 1])
            gx.index_add_(0, n_col[a:b], g_er[a:b] @ wa[r])
    return gx


# ---- the compact RGAT pair in the run-sum form ------------------------------------------------------------------------------------
def rgat_runs_reference(feat, el, er, go, srow, drow, col, num_nodes, slope=0.2, attn=None, rel_of_row=None, h0=None, nb=None,
                        keep=None):
    """het_rgat_aggregate_compact_runs / het_rgat_backward_compact_runs (include/het_amd.h) written out, in the dtype of ``feat``:
    feat [S_row,H,D], el [S_row,H], er [S_col,H], go [N,H,D]; srow / drow / col [E]: feat row, er row and destination of every edge.
    attn [R,H,D] + rel_of_row [S_row]: the fold grad_feat += grad_el (x) attn[r] and grad_attn_l.  h0 [nh,X]: h_ref = h0 + ret.
    nb: grad_bias = column sums of the first nb gradout rows.  keep [E] bool: the edges that take part (a mutation drops one).
    Returns a dict; tests/test_bf16_rows_ref.py holds it against the oracle's CompactAsOfNodeKind-4 pair."""
    if keep is not None:
        srow, drow, col = srow[keep], drow[keep], col[keep]
    dt = feat.dtype
    S_row, H, D = feat.shape
    S_col, N = er.shape[0], num_nodes
    z = el[srow] + er[drow]
    s = torch.where(z > 0, z, z * slope)
    dl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    m = torch.full((N, H), -float("inf"), dtype=dt).scatter_reduce(0, col.unsqueeze(-1).expand(-1, H), s, "amax")
    w = torch.exp(s - m[col])
    den = torch.zeros(N, H, dtype=dt).index_add(0, col, w)
    has_in = torch.zeros(N, dtype=torch.bool)
    has_in[col] = True
    lse = torch.where(den > 0, m + torch.log(den.clamp_min(1e-300 if dt == torch.float64 else 1e-30)), torch.zeros_like(den))
    a = w / den[col]
    f_e = feat[srow]
    ret = torch.zeros(N, H, D, dtype=dt).index_add(0, col, a.unsqueeze(-1) * f_e)
    wd = torch.exp(s) * dl
    res = dict(has_in=has_in, lse=lse, ret=ret, q_sum=torch.zeros(S_col, H, dtype=dt).index_add(0, drow, wd),
               q_rows=torch.zeros(S_col, H, D, dtype=dt).index_add(0, drow, wd.unsqueeze(-1) * f_e))
    if h0 is not None:
        res["nh"] = h0.shape[0]
        res["h_ref"] = h0 + ret.view(N, H * D)[:h0.shape[0]]
    g_e = go[col]
    gz = a * ((g_e * f_e).sum(-1) - (go * ret).sum(-1)[col]) * dl
    res["grad_el"] = torch.zeros(S_row, H, dtype=dt).index_add(0, srow, gz)
    res["grad_er"] = torch.zeros(S_col, H, dtype=dt).index_add(0, drow, gz)
    res["grad_feat"] = torch.zeros(S_row, H, D, dtype=dt).index_add(0, srow, a.unsqueeze(-1) * g_e)
    if attn is not None:
        res["grad_feat"] = res["grad_feat"] + res["grad_el"].unsqueeze(-1) * attn[rel_of_row]
        res["grad_attn_l"] = torch.zeros_like(attn).index_add(0, rel_of_row, res["grad_el"].unsqueeze(-1) * feat)
    if nb is not None:
        res["grad_bias"] = go.view(N, H * D)[:nb].sum(0)
    return res


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
ROWS_MATMUL_SHAPES = [(K, X) for K in (32, 64) for X in (32, 64, 128)]        # het_rows_matmul_bf16 / _backward_dw_bf16
# (H, K, D) of het_rows_matmul_heads_bf16: every (K, H*D) pair of its launcher, heads of 16, 32 and 64
HEADS_SHAPES = [(2, 32, 16), (4, 32, 16), (2, 32, 64), (1, 64, 32), (4, 64, 16), (1, 64, 64), (8, 64, 16), (2, 128, 16), (2, 128, 32),
                (4, 128, 32)]
DOT1H_SHAPES = [(H, K) for K in (32, 64) for H in (1, 2, 4, 8)]               # K >= 4 H throughout
EL_ROWS_SHAPES = [(2, 16), (1, 32), (4, 16), (2, 32), (1, 64), (8, 16), (4, 32), (2, 64), (1, 128)]  # = RUN_SHAPES of the ladder tests
LINEAR_SHAPES = [(32, 32), (64, 64), (128, 64), (32, 128), (64, 128), (128, 32)]
NODE_DX_SHAPES = [(4, 64, 16), (1, 64, 64), (2, 32, 16), (2, 64, 32), (1, 32, 32)]  # test_rgat_node_backward_dx_ladder's
NODE_SUM_WIDTHS = [(32, 64), (64, 32), (64, 64)]                              # beside the (32, 32) of the relation-count ladder


def ladder_lists(n_x, gen, distinct=False):
    """(rel_ptrs, index list [n]) over the ROW_LADDER relations: a random gather list with repeats, or distinct rows (a scatter list
    of an entry that stores plainly)."""
    rp = row_ladder_ptrs()
    n = int(rp[-1])
    assert n == sum(ROW_LADDER)
    idx = torch.randperm(n_x, generator=gen)[:n] if distinct else torch.randint(0, n_x, (n,), generator=gen)
    return rp, idx.contiguous()


# ---- the dense cases: inputs (bf16 rows drawn in fp32 and rounded once, fp32 weights) and their references ---------------------------
def _ns(**kw):
    from types import SimpleNamespace
    return SimpleNamespace(**kw)


def dense_case(K, X, seed, H=1):
    """Inputs over the row-count ladder for the entries with rows [*, K] in and [*, X] (or [*, H]) out: x bf16 [n + 17, K] behind a
    gather list with repeats, a scatter list of distinct rows of an [n + 9, .] output, gradients of both kinds, weights."""
    gen = torch.Generator().manual_seed(seed)
    rp = row_ladder_ptrs()
    R, n = rp.numel() - 1, int(rp[-1])
    Nx, No = n + 17, n + 9
    c = _ns(rp=rp, R=R, n=n, Nx=Nx, No=No, K=K, X=X, H=H)
    c.x = bf16_input(Nx, K, gen=gen)
    c.gather = torch.randint(0, Nx, (n,), generator=gen)
    c.scatter = torch.randperm(No, generator=gen)[:n].contiguous()
    c.W = torch.randn(R, K, X, generator=gen) * 0.3
    c.go32 = torch.randn(No, X, generator=gen)           # an fp32 output gradient ...
    c.gob = bf16_input(No, X, gen=gen)                   # ... and a bf16 one, read through g_rows
    c.g_rows = torch.randint(0, No, (n,), generator=gen)
    c.gw0 = torch.randn(R, K, X, generator=gen)          # what accumulate=True adds onto
    c.w1h = torch.randn(R, H, K, generator=gen) * 0.3    # the one-head row-dot's vectors
    c.go1h = torch.randn(n, H, generator=gen)
    c.gw1h0 = torch.randn(R, H, K, generator=gen)
    c.bias = torch.randn(X, generator=gen)
    return c


def gathered(c, dt, gather=True):
    return (c.x.to(dt)[c.gather] if gather else c.x.to(dt)[:c.n])


def rows_matmul_ref(c, dt, gather, rel_ptrs=None):
    return rows_matmul(c.rp if rel_ptrs is None else rel_ptrs, gathered(c, dt, gather), c.W.to(dt))


def rows_matmul_dw_ref(c, dt, gather, bf16_gradout, accumulate, rel_ptrs=None, drop_row=None):
    xs = gathered(c, dt, gather).clone()
    gs = c.gob.to(dt)[c.g_rows] if bf16_gradout else c.go32.to(dt)[:c.n]
    if drop_row is not None:
        xs[drop_row] = 0
    gw = rows_matmul_dw(c.rp if rel_ptrs is None else rel_ptrs, xs, gs, c.R)
    return gw + c.gw0.to(dt) if accumulate else gw


def rows_dot1h_ref(c, dt, rel_ptrs=None):
    return rows_dot1h(c.rp if rel_ptrs is None else rel_ptrs, gathered(c, dt), c.w1h.to(dt))


def rows_dot1h_dw_ref(c, dt, accumulate, rel_ptrs=None, drop_row=None):
    xs = gathered(c, dt).clone()
    if drop_row is not None:
        xs[drop_row] = 0
    gw = rows_dot1h_dw(c.rp if rel_ptrs is None else rel_ptrs, xs, c.go1h.to(dt), c.R)
    return gw + c.gw1h0.to(dt) if accumulate else gw


def linear_bias_ref(c, dt, bias):
    """x . W[0] (+ bias) for every row of x: the entry is then called for row ranges [lo, hi) at ladder boundaries."""
    y = c.x.to(dt) @ c.W.to(dt)[0]
    return y + c.bias.to(dt) if bias else y


def heads_case(H, K, D, seed):
    gen = torch.Generator().manual_seed(seed)
    rp = row_ladder_ptrs()
    R, n = rp.numel() - 1, int(rp[-1])
    c = _ns(rp=rp, R=R, n=n, H=H, K=K, D=D, Nx=n + 17)
    c.x = bf16_input(c.Nx, K, gen=gen)
    c.gather = torch.randint(0, c.Nx, (n,), generator=gen)
    c.W = torch.randn(R, H, K, D, generator=gen) * 0.3
    return c


def heads_ref(c, dt, rel_ptrs=None):
    return rows_matmul(c.rp if rel_ptrs is None else rel_ptrs, c.x.to(dt)[c.gather], heads_to_columns(c.W.to(dt)))


def el_rows_case(H, D, seed):
    gen = torch.Generator().manual_seed(seed)
    rp = row_ladder_ptrs()
    R, n = rp.numel() - 1, int(rp[-1])
    return _ns(rp=rp, R=R, n=n, H=H, D=D, feat=bf16_input(n, H, D, gen=gen), attn=torch.randn(R, H, D, generator=gen))


def el_rows_ref(c, dt, rel_ptrs=None):
    return el_rows(c.rp if rel_ptrs is None else rel_ptrs, c.feat.to(dt), c.attn.to(dt))


def drop_last_of(rp, rows=2049):
    """Index of the last row of the relation with ``rows`` rows."""
    r = ROW_LADDER.index(rows)
    return int(rp[r + 1]) - 1


def first_after_empty_moved(rp, two_back=False):
    """rel_ptrs with the first row of the relation after the empty one attributed to the relation before it: to the empty relation
    itself, or (two_back) to the last relation with rows in front of it."""
    r = ROW_LADDER.index(0)
    out = rp.clone()
    out[r + 1] += 1
    if two_back:
        out[r] += 1
    return out


def node_dx_case(g, H, Kd, D, self_loop=True):
    """Inputs of rgat_node_backward_dx_bf16 on the (relation, source) / (relation, destination) lists of ``g``: grad_h bf16 [N - 5, X],
    everything else fp32 (test_rgat_node_backward_dx_ladder's, the self-loop gradient rounded)."""
    R, N = g.get_num_rels(), g.get_num_nodes()
    ss = g.get_separate_unique_node_indices_single_sided()
    gen = torch.Generator().manual_seed(H + Kd)
    X = H * D
    c = _ns(R=R, N=N, H=H, K=Kd, D=D, X=X, n_loop=N - 5 if self_loop else 0, rp_row=ss["rel_ptrs_row"], n_row=ss["node_indices_row"],
            rp_col=ss["rel_ptrs_col"], n_col=ss["node_indices_col"])
    c.gh = bf16_input(c.n_loop, X, gen=gen) if self_loop else None
    c.g_rows = torch.randn(c.n_row.numel(), X, generator=gen)
    c.g_er = torch.randn(c.n_col.numel(), H, generator=gen)
    c.loop_w = torch.randn(Kd, X, generator=gen) * 0.3
    c.W = torch.randn(R, H, Kd, D, generator=gen) * 0.3
    c.wa = torch.randn(R, H, Kd, generator=gen) * 0.3
    touched = torch.zeros(N, dtype=torch.bool)
    touched[c.n_row] = True
    touched[c.n_col] = True
    c.no_rows = ~touched                                   # nodes without a row in any relation: the self-loop term only ...
    c.zero_rows = c.no_rows.clone()
    c.zero_rows[:c.n_loop] = False                         # ... or, beyond n_loop, exactly zero
    return c


def node_dx_ref(c, dt):
    return node_dx(c.N, c.n_loop, None if c.gh is None else c.gh.to(dt), c.loop_w.to(dt), c.g_rows.to(dt), c.W.to(dt), c.rp_row, c.n_row,
                   c.g_er.to(dt), c.wa.to(dt), c.rp_col, c.n_col)


def node_sum_case(g, KS, XO, seed):
    """test_node_rows_matmul_sum_relation_count's inputs: one source per relation over the (relation, source) rows of ``g`` plus one
    identity-mapped source; the maps as the device builds them (row of (relation, node) or -1)."""
    R, N = g.get_num_rels(), g.get_num_nodes()
    ss = g.get_separate_unique_node_indices_single_sided()
    rp, nodes = ss["rel_ptrs_row"], ss["node_indices_row"]
    gen = torch.Generator().manual_seed(seed)
    c = _ns(R=R, N=N, KS=KS, XO=XO, rp=rp, nodes=nodes)
    c.rows = torch.randn(nodes.numel(), KS, generator=gen)
    c.xl = torch.randn(N, KS, generator=gen)
    c.wts = [torch.randn(KS, XO, generator=gen) * 0.2 for _ in range(R + 1)]
    c.maps = torch.full((R, N), -1, dtype=torch.int64)
    for r in range(R):
        a, b = int(rp[r]), int(rp[r + 1])
        c.maps[r, nodes[a:b]] = torch.arange(a, b)
    return c


def node_sum_ref(c, dt):
    return node_rows_sum(c.N, [(c.rows.to(dt), c.maps[r], c.wts[r].to(dt)) for r in range(c.R)] + [(c.xl.to(dt), None, c.wts[c.R].to(dt))])


def move_one_bf16_unit(out, ref):
    """``out`` (bf16) with ONE element moved by one bf16 unit, away from ``ref``: the element of the largest |ref|.  One unit is more
    than 2^-8 |ref| whatever the mantissa, so the bound of check_bf16 cannot hold for it."""
    o = out.detach().clone().view(-1)
    r = ref.detach().double().view(-1)
    i = int(r.abs().argmax())
    bits = o.view(torch.int16)
    away = (float(o[i]) >= float(r[i])) == (float(o[i]) >= 0)  # moving away from ref = growing in magnitude?
    bits[i] += 1 if away else -1                            # (sign-magnitude: +1 on the bits grows the magnitude)
    return o.view(out.shape)
