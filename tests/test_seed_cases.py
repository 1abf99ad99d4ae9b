"""The seed-plan model and case table on the CPU (no GPU): the model's bipartition_tree is the
ReCom oracle's, every case of ``seed_cases.CASES`` reaches the branch it is for, every plan the
model calls ok is a plan of k connected districts inside the bounds, a plan is a function of its
own inputs, and the library's argument checks answer before any device call.
"""
import dataclasses

import networkx as nx
import numpy as np
import pytest

import recom_cases as RC
import seed_cases as SC
import seed_model
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph


# ---- the model's bipartition_tree against the oracle's -----------------------------------------
@pytest.mark.parametrize("name", ["re-root 8x8 k=2", "size 8x8 k=4", "weights 9x7 k=3"])
def test_model_bipartition_is_the_oracles(name):
    """Given each trace record's draw index, the chain id, the merged pair's membership and
    ReCom's float cut rule, the model reproduces the record's root, child and attempts; following
    the accepted records it arrives at the oracle's final state."""
    case = RC.BY_NAME[name]
    spec = case.spec
    assert name != "re-root 8x8 k=2" or case.node_repeats > 1
    eu, ev = seed_model.edge_list(spec)
    target, eps = case.pop_target, case.epsilon

    def is_cut(s):
        return abs(float(s) - target) < eps * target
    n_rec = 0
    for c in range(2):
        ref = case.oracle(c)
        assert case.chain_ok(case, ref) and len(ref["trace"]) == ref["stats"]["proposals"]
        a = case.plan(c).copy()
        for rec in ref["trace"]:
            d0, d1 = int(a[eu[rec["edge"]]]), int(a[ev[rec["edge"]]])
            assert d0 != d1
            in_m = (a == d0) | (a == d1)
            b = seed_model.bipartition(spec, in_m, int(rec["draw"]), case.chain_id_offset + c, RC.SEED,
                                       case.node_repeats, case.max_attempts, is_cut, (eu, ev))
            assert (b["root"], b["child"], b["attempts"]) == (int(rec["root"]), int(rec["child"]), int(rec["attempts"])), \
                (name, c, int(rec["draw"]))
            if rec["flags"] & 2:  # accepted: subtree(child) -> d0, the rest of M -> d1
                a[in_m] = np.where(b["subset"][in_m], d0, d1)
            n_rec += 1
        assert np.array_equal(a, ref["final"]), (name, c)
    assert n_rec >= 2 * case.steps


# ---- the case table ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.BY_NAME))
def test_case_meets_its_coverage_condition(name):
    case = SC.BY_NAME[name]
    res = case.model()
    assert len(res) == case.n_plans
    assert case.ok(case, res), (name, [(r["ok"], r["attempts"], r["trees"], r["restarts"]) for r in res])


@pytest.mark.parametrize("name", list(SC.BY_NAME))
def test_ok_plans_are_valid_and_failed_plans_are_empty(name):
    case = SC.BY_NAME[name]
    spec = case.spec
    lo, hi = case.bounds
    g = nx.Graph()
    g.add_nodes_from(range(spec.n))
    g.add_edges_from(map(tuple, spec.edges()))
    for i, r in enumerate(case.model()):
        a = r["assign"]
        if not r["ok"]:
            assert np.all(a == -1) and r["cut"] == 0 and r["nb"] == 0, (name, i)
            continue
        assert sorted(set(a.tolist())) == list(range(case.k)), (name, i)
        for d in range(case.k):
            nodes = np.nonzero(a == d)[0].tolist()
            assert nx.is_connected(g.subgraph(nodes)), (name, i, d)
            assert lo <= int(spec.pop[nodes].astype(np.int64).sum()) <= hi, (name, i, d)
        assert (r["cut"], r["nb"]) == G.cut_and_boundary(spec, a)[:2], (name, i)


def test_plan_is_a_function_of_its_own_inputs():
    """Plan G computed alone is plan G of a batch; other ids, seeds and bounds give other plans."""
    case = SC.BY_NAME["many blocks 8x8 k=2"]
    lo, hi = case.bounds
    batch = case.model()
    for i in (0, 17, 36):
        alone = seed_model.seed_plan(case.spec, case.k, lo, hi, SC.SEED, case.plan_id_offset + i)
        assert np.array_equal(alone["assign"], batch[i]["assign"])
        assert {f: alone[f] for f in alone if f != "assign"} == {f: batch[i][f] for f in batch[i] if f != "assign"}
    assert len({r["assign"].tobytes() for r in batch}) > case.n_plans // 2
    other = seed_model.seed_plan(case.spec, case.k, lo, hi, SC.SEED + 1, case.plan_id_offset)
    assert not np.array_equal(other["assign"], batch[0]["assign"])


# ---- host checks, through the library (it loads and answers these without a GPU) --------------------
def _seed(spec, k, lohi, **kw):
    return FlipGraph(spec).seed_plans(k, 3, pop_bounds=lohi, **kw)


@pytest.mark.parametrize("k", [1, 33, 0, -2])
def test_host_refuses_k_out_of_range(k):
    with pytest.raises(ValueError, match=r"fc_graph_seed_plans: k must be in \[2, 32\]"):
        _seed(RC.grid(8, 8), k, (0, 64))


def test_host_refuses_impossible_bounds():
    spec = RC.grid(8, 8)
    with pytest.raises(ValueError, match="pop_lo 17 > pop_hi 16"):
        _seed(spec, 4, (17, 16))
    with pytest.raises(ValueError, match=r"k \* pop_lo = 4 \* 17 exceeds the population total 64"):
        _seed(spec, 4, (17, 40))
    with pytest.raises(ValueError, match=r"k \* pop_hi = 4 \* 15 is below the population total 64"):
        _seed(spec, 4, (3, 15))
    with pytest.raises(ValueError, match="max_restarts must be below 2\\^24"):
        _seed(spec, 4, (15, 17), max_restarts=1 << 24)
    with pytest.raises(ValueError, match="must be >= 0"):
        _seed(spec, 4, (15, 17), max_attempts=-1)
    with pytest.raises(ValueError, match="exactly one of pop_bounds"):
        FlipGraph(spec).seed_plans(4, 3)
    with pytest.raises(ValueError, match="exactly one of pop_bounds"):
        FlipGraph(spec).seed_plans(4, 3, pop_bounds=(15, 17), percent=0.1)


def test_host_refuses_what_the_tree_kernel_cannot_hold():
    with pytest.raises(NotImplementedError, match=r"spanning tree in LDS \(n <= 8000\)"):
        _seed(RC.grid(127, 63), 2, (0, 8001))  # n = 8001
    with pytest.raises(NotImplementedError, match="population total 4294967296 exceeds INT32_MAX = 2147483647"):
        _seed(RC.overweight_grid(), 2, (0, 2 ** 40))
    two = nx.Graph([(0, 1), (2, 3)])
    spec = G.from_networkx(two, pos={i: (float(i), 0.0) for i in range(4)})
    spec = dataclasses.replace(spec, pop=np.ones(4, dtype=np.int32))
    with pytest.raises(NotImplementedError, match="the graph must be connected"):
        _seed(spec, 2, (1, 3))


def test_abi_structs_match_the_header():
    import ctypes
    import os
    from flipcomplexityempirical_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flipchain.h")).read()
    for name in ("fc_seed_params_init", "fc_graph_seed_plans", "fc_seed_kernel_name"):
        assert name in _lib.EXPORTED and f"int {name}(" in hdr
    assert ctypes.sizeof(_lib.SeedParams) == 64 and ctypes.sizeof(_lib.SeedStats) == 32
    L = _lib.load()
    prm = _lib.SeedParams()
    assert L.fc_seed_params_init(ctypes.byref(prm), ctypes.sizeof(prm)) == _lib.FC_OK
    assert (prm.struct_size, prm.abi_version, prm.k, prm.pop_lo, prm.pop_hi) == (64, _lib.FC_ABI_VERSION, 2, 0, 2 ** 63 - 1)
    assert L.fc_seed_params_init(ctypes.byref(prm), 48) == _lib.FC_ERR_ARG
    assert L.fc_graph_seed_plans(None, None, 0, None, None, None) == _lib.FC_ERR_ARG
    prm.struct_size = 48  # a caller built against another layout
    fg = FlipGraph(RC.grid(4, 4))
    assert L.fc_graph_seed_plans(fg.handle, ctypes.byref(prm), 0, None, None, None) == _lib.FC_ERR_ARG
    assert b"fc_seed_params_init" in L.fc_last_error()
