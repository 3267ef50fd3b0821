"""Cases and comparison of the RGCN compact-aggregation and HGT softmax / message-aggregation pins (tests/golden/*_rgcn_hgt.npz:
outputs of the reference's own ref_rgcn.py / ref_hgt.py, tests/golden/make_golden.py::main_rgcn_hgt), shared by
tests/test_rgcn_hgt_golden.py (oracle, CPU) and tests/test_gpu_rgcn_hgt_golden.py (HIP).  Reads the .npz files and recipe.py only.

Tolerances (the project's own):
  SUM   results that are sums over edges: tests.util.assert_close at its defaults (rtol 2e-4, atol 2e-5 * max(1, max |ref|)) -- the
        reference adds in fp32 in its own order;
  EDGE  per-edge products with no sum (hgtab_grad_message; hgts_a given the sum): rtol 1e-6 / atol 1e-7 for the fp64 oracle, rtol
        1e-5 / atol 1e-6 for HIP, as check_round5_gat_pins holds ``exp``.  Why the oracle's bound can hold for hgts_a: the
        generator rounds exp(score * mu) to fp32 (1 ulp), hands the reference m / mu, which multiplies by mu again (2 roundings),
        divides by a sum that was added up in fp64 and rounded once, and rounds the quotient: at most 5 roundings of 2^-24 = 3e-7
        relative, against an oracle that rounds nothing."""
import json

import torch

from het_amd.graph import HetGraph
from het_amd.synth import IntegratedCOO
from tests.conftest import load_golden
from tests.golden import recipe
from tests.util import assert_close, permute_eids

GRAPHS = ("toy", "mag01_slice", "mag01_full")
EDGE_TOL = {"oracle": (1e-6, 1e-7), "hip": (1e-5, 1e-6)}
_cases = {}


def _coo(which):
    if which == "mag01_full":
        row, col, rel, eids, n, R = recipe.integrated_coo(load_golden("mag01_full.npz")["coo"])
    else:
        gold = load_golden({"toy": "toy.npz", "mag01_slice": "mag01_slice.npz"}[which])
        row, col, rel, eids, n, R = gold["row"], gold["col"], gold["rel"], gold["eids"], int(gold["num_nodes"]), int(gold["num_rels"])
    return IntegratedCOO(n, R, torch.tensor([0, n]), row, col, rel, eids)


def _graph(which, permuted):
    g = HetGraph.from_integrated_coo(_coo(which))
    g.get_in_csr(), g.get_out_csr()
    if permuted:
        permute_eids(g, 4242)
    return g


def load_case(which, permuted=False):
    """{"which", "n", "R", "E", "g" (CPU HetGraph: the layouts of our builders, equal to the reference builders' -- tests/
    test_layouts_golden.py, tests/test_mag01_full.py -- with canonical eids, or with every layout renumbered by one random
    permutation), "inp" (position-ordered float inputs, regenerated and checked against the digests of the fixture), "rows"
    (recipe.pinned_rows, checked likewise), "gold"}.  Built once per (graph, numbering) and shared: do not modify."""
    if (which, permuted) in _cases:
        return _cases[which, permuted]
    gold = load_golden(which + "_rgcn_hgt.npz")
    dig = json.loads(str(gold["digests_json"]))
    g = _graph(which, permuted)
    s = g.get_separate_coo_original()
    n, R, E = g.get_num_nodes(), g.get_num_rels(), g.get_num_edges()
    inp = recipe.rgcn_hgt_inputs(which, E, n, R)
    for k, v in inp.items():
        assert recipe.digest(v) == dig["input_" + k], f"regenerated input {k} differs from the one the reference ran on"
        if k in gold:  # (the toy fixture also holds its inputs in full)
            assert torch.equal(gold[k], v), k
    rows = recipe.pinned_rows(which, s["row_indices"], s["col_indices"], n)
    for k, v in rows.items():
        assert recipe.digest(v) == dig["rows_" + k], f"pinned rows {k} differ from the ones the fixture stores"
    case = {"which": which, "n": n, "R": R, "E": E, "g": g, "inp": inp, "rows": rows, "gold": gold, "permuted": permuted}
    _cases[which, permuted] = case
    return case


def by_id(x_pos, eids):
    """Edge data stored by edge id: out[eids[p]] = x_pos[p]."""
    out = torch.empty_like(x_pos)
    out[eids] = x_pos
    return out


def rgcn_dict(g, direct):
    if direct:
        return {"inverse_indices_row": g.get_separate_unique_node_indices_single_sided_inverse_idx()["inverse_indices_row"]}
    ss = g.get_separate_unique_node_indices_single_sided()
    return {"rel_ptrs_row": ss["rel_ptrs_row"], "node_indices_row": ss["node_indices_row"]}


def pin_close(actual, case, key, side, edge=False, what=""):
    """``actual`` (whole graph; node rows or position-ordered edge rows) on the rows the fixture stores against the reference's
    ``key``; prints the largest deviation before it asserts."""
    ref = case["gold"][key]
    got = actual.detach().cpu().double()[case["rows"][recipe.PIN_ROWS[key]]]
    d = (got - ref.double()).abs()
    scale = float(ref.abs().max())
    print(f"PIN {case['which']:<11} {key:<21} {side:<6} {what:<28} max |d| {float(d.max()):.3e}  max |d| / max |ref| {float(d.max()) / scale:.3e}")
    if edge:
        rtol, atol = EDGE_TOL[side]
        torch.testing.assert_close(got, ref.double(), rtol=rtol, atol=atol, msg=lambda m: f"{key} {what}: {m}")
    else:
        assert_close(got, ref, what=f"{key} {what}")
