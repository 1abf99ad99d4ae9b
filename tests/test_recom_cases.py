"""The ReCom case table on the CPU: every case reaches the branch it is for, and the oracle's
individual steps are ReCom moves by the definition.

``recom_cases.CASES`` drives the device parity test (test_recom_edges_gpu.py).  Parity with
``oracle/recomref.c`` is worth what the oracle is worth, so each of its trace records is checked
here against the states before and after it with networkx and numpy only: the random stream is
counter-based, so ``recom_run(n_steps=s)`` for s = 0 .. S is the state after every step.
"""
import networkx as nx
import numpy as np
import pytest

import recom_cases as RC

WALK_STEPS = 40  # S: states recomputed per chain


def _chains(case):
    """Chains whose coverage is checked: offset + {0, 1, 2} at the least, and every chain of the
    case beyond that (cheap), since the device test asserts the condition on each of its chains
    and a ``run_ok`` condition speaks of all of them together."""
    return range(max(3, case.n_chains))


@pytest.mark.parametrize("name", list(RC.BY_NAME))
def test_case_reaches_its_branch(name):
    """A failure here means the case is wrong (parameters, seed or step count), not the kernel."""
    case = RC.BY_NAME[name]
    refs = [case.oracle(c) for c in _chains(case)]
    for c, ref in enumerate(refs):
        assert case.chain_ok(case, ref), (name, case.chain_id_offset + c, ref["stats"])
        assert len(ref["trace"]) == ref["stats"]["proposals"] - (ref["stats"]["stuck"] and not case.max_draws), name
    if case.run_ok is not None:
        assert case.run_ok(case, refs), name
    if not case.trace_cap:
        assert max(r["stats"]["proposals"] for r in refs) <= case.room, name


def test_case_graphs_build_on_the_host():
    """The host graph builder takes every case's graph, and the Delaunay case is the one with
    neighbour rows of 16."""
    from flipcomplexityempirical_amd.engine import FlipGraph
    for case in RC.CASES:
        fg = FlipGraph(case.spec)
        assert fg.n == case.spec.n and fg.n_edges == case.spec.n_edges, case.name
        assert f"fc::recom_kernel<{fg.info['ring_max']}>" == case.kernel, case.name
        fg.close()


def test_run_create_refuses_what_the_kernel_cannot_hold():
    """Host-side checks of fc_run_create (FC_ERR_UNSUPPORTED), made before a device is touched: a
    population total past INT32_MAX (int32 subtree sums, bit 31 the subset mark) and n > 8000."""
    with pytest.raises(NotImplementedError, match="INT32_MAX = 2147483647"):
        RC.create_run(RC.overweight_grid())
    with pytest.raises(NotImplementedError, match="n <= 8000"):
        RC.create_run(RC.grid(127, 63))  # n = 8001


def _connected(g, nodes):
    return len(nodes) > 0 and nx.is_connected(g.subgraph(nodes))


def _check_record(case, g, edges, pop, rec, before, after, lo, hi):
    """One trace record between the states before and after it, from the definition of a ReCom move."""
    u, v = edges[rec["edge"]]
    d0, d1 = before[u], before[v]
    assert d0 != d1, "edge is not a cut edge of the state before"
    in_m = (before == d0) | (before == d1)
    flags = int(rec["flags"])
    assert flags in (1, 3, 8)
    assert in_m[rec["root"]] and in_m[rec["child"]] and rec["root"] != rec["child"]
    assert 1 <= rec["attempts"] <= case.max_attempts
    if flags & 2:
        assert np.array_equal(after[~in_m], before[~in_m]), "a node outside the merged pair moved"
        part0, part1 = np.nonzero(in_m & (after == d0))[0], np.nonzero(in_m & (after == d1))[0]
        assert len(part0) + len(part1) == int(in_m.sum()), "the new parts do not partition the merged pair"
        assert _connected(g, part0) and _connected(g, part1)
        assert after[rec["child"]] == d0  # subtree(child) takes the first district of the edge
        p0, p1 = int(pop[part0].sum()), int(pop[part1].sum())
        assert abs(float(p0) - case.pop_target) < case.epsilon * case.pop_target
        assert lo <= p0 <= hi and lo <= p1 <= hi
    else:
        # flags == 1 (cut_accept said no) or 8 (the Validator said no): the state stays.  For 8
        # some part of the proposed state left the bounds; that state is not recorded, so
        # nothing stronger can be checked here
        assert np.array_equal(after, before)
    assert rec["cut"] == int((after[edges[:, 0]] != after[edges[:, 1]]).sum())


@pytest.mark.parametrize("name", [c.name for c in RC.CASES if c.walk])
def test_oracle_steps_are_recom_moves(name):
    case = RC.BY_NAME[name]
    spec = case.spec
    assert spec.n <= 256
    g = nx.Graph()
    g.add_nodes_from(range(spec.n))
    edges = spec.edges()
    g.add_edges_from(edges.tolist())
    pop = spec.pop.astype(np.int64)
    for c in range(3):
        lo, hi = case.chain_bounds(c)
        full = case.oracle(c, n_steps=min(case.steps, WALK_STEPS))
        n_steps = full["stats"]["steps"]
        states = [case.oracle(c, n_steps=s)["final"] for s in range(n_steps)] + [full["final"]]
        assert np.array_equal(states[0], case.plan(c))
        s = 0
        for rec in full["trace"]:
            valid = int(rec["flags"]) != 8
            _check_record(case, g, edges, pop, rec, states[s], states[s + valid], lo, hi)
            s += valid
        assert s == n_steps
        for st in states:  # every state is a plan of k contiguous districts inside the bounds
            pops = np.bincount(st, weights=pop, minlength=case.k)
            assert lo <= pops.min() and pops.max() <= hi
            assert all(_connected(g, np.nonzero(st == d)[0]) for d in range(case.k))
