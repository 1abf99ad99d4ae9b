"""Plan samples, the parts that need no GPU: the host model (tests/plans_model.py)
against a per-yield recomputation of an oracle chain's trace; ``engine.sample_times``; the argument
checks ``FlipRun.sample_plans`` makes before the library call; the new names in the header and the
binding; ``MarkovChain.run(sample_every=...)`` argument handling."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import plans_model as PM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipRun, sample_times
from test_splits import _oracle_chain


# ---- the model against brute force -------------------------------------------------------------

def _cut_and_boundary(a, edges):
    """|cut| and |B| (the nodes with a neighbour in another district) of one assignment, from the
    definition."""
    m = a[edges[:, 0]] != a[edges[:, 1]]
    return int(m.sum()), int(np.unique(edges[m]).size)


@pytest.mark.parametrize("k", [2, 4])
def test_model_against_brute_force(cref, k):
    steps = 1200
    spec, a0, ev, final = _oracle_chain(cref, k, steps)
    assert len(ev) > 200
    edges = spec.edges()
    pop = np.arange(1, spec.n + 1, dtype=np.int64)  # distinct populations: a wrong node shows in pops
    # every yield's assignment, |cut| and |B|, event by event in Python
    a = a0.astype(np.int64).copy()
    per_yield, nxt = [], 0
    for t in range(steps + 1):
        while nxt < len(ev) and ev[nxt, 0] <= t:
            a[ev[nxt, 1]] = ev[nxt, 4]
            nxt += 1
        per_yield.append((a.copy(),) + _cut_and_boundary(a, edges))
    assert np.array_equal(per_yield[-1][0], final)
    # the log's own |cut| and |B| are those of the recomputed states
    for t, _, c, b, _ in ev[:50]:
        assert (c, b) == per_yield[t][1:]
    for t0 in (0, 500):  # the whole run, and a window that starts mid-run
        a_start, cut0, nb0 = per_yield[t0]
        w = ev[ev[:, 0] > t0]
        first = int(w[0, 0])
        patterns = {"every": np.arange(t0, steps + 1), "stride7": np.arange(t0, steps + 1, 7),
                    "stride500": np.arange(t0, steps + 1, 500), "first": np.array([t0]), "last": np.array([steps]),
                    "before_first_event": np.arange(t0, first), "on_and_around_events": np.unique(
                        np.concatenate([w[:40, 0] - 1, w[:40, 0], w[-3:, 0]])),
                    "none": np.zeros(0, dtype=np.int64)}
        for name, times in patterns.items():
            m = PM.replay(a_start, w, t0, steps, cut0, nb0, pop, times, k)
            assert m["plans"].shape == (times.size, spec.n) and m["pops"].shape == (times.size, k), name
            for j, t in enumerate(times):
                at, ct, bt = per_yield[t]
                assert np.array_equal(m["plans"][j], at), (name, t)
                assert (int(m["cut"][j]), int(m["nb"][j])) == (ct, bt), (name, t)
                assert int(m["dist0"][j]) == sum(int(x != y) for x, y in zip(at, a_start)), (name, t)
                assert m["pops"][j].tolist() == [int(pop[at == d].sum()) for d in range(k)], (name, t)
            if name == "first":
                assert m["dist0"].tolist() == [0] and np.array_equal(m["plans"][0], a_start)
            if name == "before_first_event":
                assert times.size > 0 and (m["dist0"] == 0).all() and (m["cut"] == cut0).all()
            if name == "every":
                assert m["repeat_between"] == 0  # one yield holds at most one event
            if name == "stride7":
                assert m["chunk_same_node"] > 0 and m["repeat_between"] > 0
                assert len(set(m["dist0"].tolist())) > 10


def test_model_event_order_on_one_node():
    """Three events on node 2 inside one interval: the last one's target holds."""
    ev = np.array([[3, 2, 5, 4, 1], [4, 2, 6, 5, 2], [6, 2, 7, 6, 0], [7, 1, 8, 7, 2]])
    m = PM.replay([0, 0, 0, 0], ev, 1, 9, 4, 3, [1, 10, 100, 1000], [1, 2, 3, 5, 6, 9], 3)
    assert m["plans"][:, 2].tolist() == [0, 0, 1, 2, 0, 0] and m["plans"][:, 1].tolist() == [0, 0, 0, 0, 0, 2]
    assert m["cut"].tolist() == [4, 4, 5, 6, 7, 8] and m["nb"].tolist() == [3, 3, 4, 5, 6, 7]
    assert m["dist0"].tolist() == [0, 0, 1, 1, 0, 1]
    assert m["pops"].tolist() == [[1111, 0, 0]] * 2 + [[1011, 100, 0], [1011, 0, 100], [1111, 0, 0], [1101, 0, 10]]
    assert m["chunk_same_node"] == 2 and m["repeat_between"] == 0
    m = PM.replay([0, 0, 0, 0], ev, 1, 9, 4, 3, [1, 1, 1, 1], [2, 6], 3)
    assert m["plans"][1].tolist() == [0, 0, 0, 0] and m["repeat_between"] == 1


# ---- sample_times and the Python argument checks -----------------------------------------------

def test_sample_times():
    assert sample_times(0, 10, 5).tolist() == [0, 5, 10] and sample_times(0, 10, 5).dtype == np.int64
    assert sample_times(0, 9, 5).tolist() == [0, 5]
    assert sample_times(1000, 3000, 1000).tolist() == [1000, 2000, 3000]
    assert sample_times(1000, 3000, 700, first=1500).tolist() == [1500, 2200, 2900]
    assert sample_times(1000, 3000, 700, first=0).tolist() == [0, 700, 1400, 2100, 2800]
    assert sample_times(4, 4, 1).tolist() == [4] and sample_times(5, 4, 1).tolist() == []
    assert sample_times(0, 1000, 50).tolist() == [i for i in range(1001) if i % 50 == 0]
    for every in (0, -1):
        with pytest.raises(ValueError, match="every"):
            sample_times(0, 10, every)


def test_python_argument_errors():
    """The checks of ``FlipRun.sample_plans`` that come before the library call (a stand-in run:
    none of these reaches the handle)."""
    run = types.SimpleNamespace(n_chains=3, handle=None)
    call = functools.partial(FlipRun.sample_plans, run)
    for bad in ([0.0, 1.0], np.array([0.5]), ["a"]):
        with pytest.raises(ValueError, match="times must be integers"):
            call(times=bad)
    for bad in (np.zeros((2, 2), dtype=np.int64), 5):
        with pytest.raises(ValueError, match="times must be one-dimensional"):
            call(times=bad)
    for bad in ([3, 3], [0, 5, 4], [2, 1]):
        with pytest.raises(ValueError, match="times must be strictly increasing"):
            call(times=bad)
    with pytest.raises(ValueError, match="either times or every"):
        call()
    with pytest.raises(ValueError, match="either times or every"):
        call(times=[1], every=2)


def test_names_in_header_and_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flipchain.h")) as f:
        header = f.read()
    L = _lib.load()
    assert "fc_run_sample_plans" in _lib.EXPORTED and "int fc_run_sample_plans(" in header
    assert L.fc_run_sample_plans.restype is ctypes.c_int and len(L.fc_run_sample_plans.argtypes) == 10
    assert "fc_run_sample_plans_ms" in _lib.EXPORTED and "int fc_run_sample_plans_ms(" in header
    assert L.fc_run_sample_plans_ms.restype is ctypes.c_int and L.fc_run_sample_plans_ms(None, None, None) == _lib.FC_ERR_ARG
    assert "#define FC_ABI_VERSION 5u" in header and _lib.FC_ABI_VERSION == 5
    from flipcomplexityempirical_amd import build
    assert "fc_plans.hip" in build.SOURCES and "fc_plans.h" in build.HEADERS
    assert L.fc_run_sample_plans(None, 0, 1, 0, None, None, None, None, None, None) == _lib.FC_ERR_ARG
    assert b"fc_run_sample_plans" in L.fc_last_error()


# ---- MarkovChain.run(sample_every=...) ----------------------------------------------------------

def _partition():
    g = G.sec11_nx()
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
           "base": lambda p: 1.0}
    return C.Partition(g, assignment=G.sec11_plan(0, sorted(g.nodes())), updaters=ups)


def test_sample_every_argument_handling():
    part = _partition()
    pb = C.within_percent_of_ideal_population(part, 0.1)
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, pb]), C.cut_accept, part,
                       total_steps=100)
    for bad in (0, -5, 2.5, "10", True):  # refused before any device work
        with pytest.raises(ValueError, match="sample_every"):
            mc.run(sample_every=bad)
    # a ReCom chain keeps no flip log
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.05, node_repeats=1)
    rc = C.MarkovChain(tree, C.Validator([pb]), C.always_accept, part, total_steps=10)
    with pytest.raises(ValueError, match="ReCom"):
        rc.run(sample_every=5)
    # a result without samples
    fields = C.ChainResult.__dataclass_fields__
    assert fields["plans"].default is None
    res = C.ChainResult(
        steps=0, proposals=0, accepted=0, waits_sum=0, rce_sum=0, rbn_sum=0, cut_hist=np.zeros(0), nb_hist=np.zeros(0),
        cut_times={}, num_flips={}, part_sum={}, last_flipped={}, lognum_flips={}, final_assignment={})
    assert res.plans is None
    with pytest.raises(ValueError, match="sample_every"):
        list(res.sampled())
    with pytest.raises(ValueError, match="sample_every"):
        res.save_plans("nowhere")
