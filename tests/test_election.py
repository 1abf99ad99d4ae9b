"""Election series, the parts that need no GPU: the per-yield rule
``fc_election_eval`` (the code the device runs) against a direct statement of it; the host model
(tests/election_model.py) against a brute-force recomputation of every yield of an oracle chain;
the host-side ``Election`` / ``Tally`` updaters; and the ``GraphSpec.columns`` plumbing."""
import ctypes
import json

import networkx as nx
import numpy as np
import pytest

import election_model as EM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.chain import Election, Partition, Tally
from oracle.flipref import events_from_trace

I64 = ctypes.POINTER(ctypes.c_int64)


def _eval(a, b):
    a = np.ascontiguousarray(a, dtype=np.int64)
    b = np.ascontiguousarray(b, dtype=np.int64)
    seats, gap = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = _lib.load().fc_election_eval(int(a.size), a.ctypes.data_as(I64), b.ctypes.data_as(I64),
                                      ctypes.byref(seats), ctypes.byref(gap))
    return rc, int(seats.value), int(gap.value)


def _rule(a, b):
    """The issue's definition, in Python integers."""
    seats = gap = 0
    for x, y in zip((int(v) for v in a), (int(v) for v in b)):
        if x > y:
            seats += 1
            gap += 3 * y - x
        elif x < y:
            gap += y - 3 * x
    return seats, gap


def test_election_eval_against_the_rule():
    rng = np.random.default_rng(5)
    top = 2 ** 31 - 1
    for k in range(1, 33):
        cases = [(rng.integers(0, 6, k), rng.integers(0, 6, k)),            # small: ties are frequent
                 (rng.integers(0, 10 ** 6, k), rng.integers(0, 10 ** 6, k)),
                 (np.zeros(k, dtype=np.int64), rng.integers(0, 100, k)),    # a = 0
                 (rng.integers(0, 100, k), np.zeros(k, dtype=np.int64)),    # b = 0
                 (np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)),
                 (np.full(k, top), rng.integers(top - 3, top + 1, k)),      # near 2^31
                 (rng.integers(top - 3, top + 1, k), np.full(k, top)),
                 (np.full(k, top), np.zeros(k, dtype=np.int64)),
                 (np.zeros(k, dtype=np.int64), np.full(k, top))]
        a = rng.integers(0, 50, k)
        cases.append((a, a.copy()))                                         # every district tied
        for a, b in cases:
            rc, seats, gap = _eval(a, b)
            assert rc == _lib.FC_OK
            assert (seats, gap) == _rule(a, b), (k, a, b)
    # the doubled units: gap / (2 V) is (wasted_B - wasted_A) / V on a yield without a tie
    a, b = np.array([60, 30, 45]), np.array([40, 70, 55])
    _, seats, gap = _eval(a, b)
    wasted_a = (60 - 50) + 30 + 45
    wasted_b = 40 + (70 - 50) + (55 - 50)
    assert seats == 1 and gap == 2 * (wasted_b - wasted_a)


def test_election_eval_arguments():
    L = _lib.load()
    one = np.ones(1, dtype=np.int64)
    assert _eval(np.zeros(0), np.zeros(0))[0] == _lib.FC_ERR_ARG
    assert _eval(np.zeros(33), np.zeros(33))[0] == _lib.FC_ERR_ARG
    assert _eval([-1], [0])[0] == _lib.FC_ERR_ARG
    assert _eval([0], [2 ** 31])[0] == _lib.FC_ERR_ARG
    assert L.fc_election_eval(1, None, one.ctypes.data_as(I64), None, None) == _lib.FC_ERR_ARG
    assert L.fc_election_eval(1, one.ctypes.data_as(I64), one.ctypes.data_as(I64), None, None) == _lib.FC_OK


# ---- the model against brute force ------------------------------------------------------------

def _oracle_chain(cref, steps=1500):
    spec = G.grid_graph(12, 11)
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), 2, 0.5)
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    r = cref.run(spec, a0, base=1.0, pop_lo=lo, pop_hi=hi, seed=11, chain_id=0, n_steps=steps, k=2, labels=[-1, 1],
                 log1mp=G.log1mp_table(spec.n, 2), trace_cap=64 * steps)
    return spec, a0, events_from_trace(r["trace"]), r["final"]


def test_model_against_brute_force(cref):
    steps = 1500
    spec, a0, ev, final = _oracle_chain(cref, steps)
    assert len(ev) > 300
    cols = np.random.default_rng(8).integers(0, 2, (spec.n, 3))  # 0 / 1 votes: seats change, ties occur
    elections = [(0, 1), (2, 0)]
    k = 2
    # the gap range of this chain by a first pass without edges, then edges inside and around it
    m0 = EM.replay(a0, ev[:, 0], ev[:, 1], ev[:, 4], 0, steps, cols, elections, [], k)
    edges = EM.spanning_edges(m0["gap_range"])
    for t0 in (0, 700):  # the whole run, and a window that starts mid-run
        # window-start state and the events inside the window
        a_start = a0.astype(np.int64).copy()
        for t, v, _, _, tg in ev[ev[:, 0] <= t0]:
            a_start[v] = tg
        w = ev[ev[:, 0] > t0]
        m = EM.replay(a_start, w[:, 0], w[:, 1], w[:, 4], t0, steps, cols, elections, edges, k)
        assert m["yields"] == steps - t0 + 1
        # brute force: every yield's assignment and tallies from scratch
        tally_sum = np.zeros((k, 3), dtype=np.int64)
        seats_hist = np.zeros((2, k + 1), dtype=np.int64)
        wins_sum = np.zeros((2, k), dtype=np.int64)
        gap_sum = [0, 0]
        gap_hist = np.zeros((2, edges.size + 1), dtype=np.int64)
        ties = 0
        a = a0.astype(np.int64).copy()
        nxt = 0
        for t in range(steps + 1):
            while nxt < len(ev) and ev[nxt, 0] <= t:
                a[ev[nxt, 1]] = ev[nxt, 4]
                nxt += 1
            if t < t0:
                continue
            S = [[int(cols[a == d, j].sum()) for j in range(3)] for d in range(k)]
            tally_sum += np.asarray(S)
            tie = False
            for e, (ca, cb) in enumerate(elections):
                seats = gap = 0
                for d in range(k):
                    x, y = S[d][ca], S[d][cb]
                    if x > y:
                        seats += 1
                        wins_sum[e, d] += 1
                        gap += 3 * y - x
                    elif x < y:
                        gap += y - 3 * x
                    else:
                        tie = True
                seats_hist[e, seats] += 1
                gap_sum[e] += gap
                gap_hist[e, sum(1 for x in edges if x <= gap)] += 1
            ties += tie
        assert np.array_equal(a, final) and np.array_equal(m["final"], final)
        assert np.array_equal(m["tally_now"], np.asarray(S))
        assert np.array_equal(m["tally_sum"], tally_sum)
        assert np.array_equal(m["seats_hist"], seats_hist)
        assert np.array_equal(m["wins_sum"], wins_sum)
        assert list(m["gap_sum"]) == gap_sum
        assert np.array_equal(m["gap_hist"], gap_hist)
        assert m["ties"] == ties > 0 and (m["seats_hist"] > 0).sum(axis=1).min() >= 2
        assert (m["gap_hist"].sum(axis=1) == m["yields"]).all() and (m["seats_hist"].sum(axis=1) == m["yields"]).all()
        assert (m["gap_hist"] > 0).sum(axis=1).min() >= 3  # the edges do split the gap range


# ---- host updaters and the column plumbing ------------------------------------------------------

def _voting_graph():
    g = nx.grid_graph([4, 3])
    rng = np.random.default_rng(3)
    for nd in g.nodes:
        g.nodes[nd].update(population=1, D=int(rng.integers(0, 9)), R=int(rng.integers(0, 9)))
    return g


def test_election_and_tally_updaters():
    g = _voting_graph()
    plan = {nd: (1 if nd[0] >= 2 else -1) for nd in g.nodes}
    part = Partition(g, plan, {"D": Tally("D"), "votes": Tally(["D", "R"]), "E": Election("E", {"Dem": "D", "Rep": "R"})})
    res = part["E"]
    for lab in (-1, 1):
        d = sum(g.nodes[nd]["D"] for nd in g.nodes if plan[nd] == lab)
        r = sum(g.nodes[nd]["R"] for nd in g.nodes if plan[nd] == lab)
        assert part["D"][lab] == d and part["votes"][lab] == d + r
        assert res.totals_for_party["Dem"][lab] == d and res.totals_for_party["Rep"][lab] == r
        assert res.totals(lab) == d + r
        assert res.won("Dem", lab) == (d > r) and res.won("Rep", lab) == (r > d)
    a = np.array([res.totals_for_party["Dem"][lab] for lab in (-1, 1)])
    b = np.array([res.totals_for_party["Rep"][lab] for lab in (-1, 1)])
    seats, gap = _rule(a, b)
    assert res.seats("Dem") == seats and res.seats("Rep") == _rule(b, a)[0]
    assert res.efficiency_gap() == pytest.approx(gap / (2 * (a.sum() + b.sum())), abs=1e-15)
    # a flipped partition re-evaluates
    child = part.flip({(2, 0): -1})
    assert child["E"].totals_for_party["Dem"][-1] == a[0] + g.nodes[(2, 0)]["D"]
    with pytest.raises(NotImplementedError):
        Election("E3", {"A": "D", "B": "R", "C": "population"})
    with pytest.raises(KeyError):
        res.seats("Green")


def test_graphspec_columns():
    g = _voting_graph()
    spec = G.from_networkx(g, columns=("D", "R"))
    assert set(spec.columns) == {"D", "R"}
    for name in ("D", "R"):
        assert spec.columns[name].dtype == np.int64
        assert [int(x) for x in spec.columns[name]] == [g.nodes[nd][name] for nd in spec.nodes]
    assert G.from_networkx(g).columns == {} and G.grid_graph(3, 3).columns == {}
    # through JSON (node ids come back as tuples), both layouts
    for data in (nx.adjacency_data(g), nx.node_link_data(g, edges="links")):
        back = G.from_json(json.loads(json.dumps(data)), columns=["R"])
        assert back.nodes == spec.nodes and np.array_equal(back.columns["R"], spec.columns["R"])
    with pytest.raises(ValueError):
        G.from_networkx(g, columns=("missing",))
    g.nodes[(0, 0)]["D"] = 1.5
    with pytest.raises(ValueError):
        G.from_networkx(g, columns=("D",))
