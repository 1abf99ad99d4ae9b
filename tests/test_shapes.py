"""Compactness series, the parts that need no GPU: the score ``fc_shape_score`` (the
code the device runs) against Python integers; the host model (tests/shape_model.py) against a
brute-force recomputation of every yield of an oracle chain; the new names in the header and the
binding; the host-side ``Compactness`` updater and ``unit_square_shapes``."""
import ctypes
import math
import os

import networkx as nx
import numpy as np
import pytest

import shape_model as SM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.chain import Compactness, Partition
from oracle.flipref import events_from_trace

TOP = 2 ** 31 - 1


def _score(area, perim):
    q = ctypes.c_int64(-7)
    rc = _lib.load().fc_shape_score(int(area), int(perim), ctypes.byref(q))
    return rc, int(q.value)


def _rule(area, perim):
    """The issue's definition, in Python integers."""
    return min(2 ** 20 * area // perim ** 2, TOP) if perim else 0


def test_shape_score_against_python_integers():
    cases = [(0, 0), (5, 0), (TOP, 0), (0, 1), (0, 7), (0, TOP),          # P = 0 and A = 0
             (1, 1), (2047, 1), (2048, 1), (2049, 1), (TOP, 1), (TOP, 2),   # the clamp: 2^20 A >= 2^31 P^2
             (8191, 2), (8192, 2), (TOP, 1023), (TOP, 1024), (TOP, 1025),
             (TOP, TOP), (TOP - 1, TOP), (1, TOP), (TOP, TOP - 1), (1, 1024), (1, 1025)]
    # around exact quotients: 2^20 A = q P^2 + r for r = -1, 0, 1 needs P^2 | 2^20 (A 2^20 + r is
    # not reachable for r != 0), so take P a power of two and areas one off a multiple of P^2 / 2^20
    for p in (1024, 2048, 4096, 32768):
        step = p * p // 2 ** 20
        for q in (1, 2, 3, 1000, TOP // step):
            cases += [(q * step - 1, p), (q * step, p), (min(q * step + 1, TOP), p)]
    for p in (3, 7, 1000, 12345, 46341, 10 ** 6):  # P^2 not a divisor: floor of an inexact quotient
        for x in (1, 2, p, p * p // 2 ** 20, p * p // 2 ** 20 + 1, p * p, 10 ** 9):
            cases += [(min(max(x + dx, 0), TOP), p) for dx in (-1, 0, 1)]
    rng = np.random.default_rng(6)
    cases += [(int(a), int(p)) for a, p in zip(rng.integers(0, TOP + 1, 2000), rng.integers(0, TOP + 1, 2000))]
    cases += [(int(a), int(p)) for a, p in zip(rng.integers(0, 10 ** 4, 2000), rng.integers(0, 400, 2000))]
    for a, p in cases:
        assert 0 <= a <= TOP and 0 <= p <= TOP
        rc, q = _score(a, p)
        assert rc == _lib.FC_OK and q == _rule(a, p) == SM.score(a, p), (a, p, q)
    # the units: 4 pi Q / 2^20 is the Polsby-Popper score rounded down to 4 pi / 2^20
    _, q = _score(100, 40)  # a 10 x 10 square of unit cells
    assert q == 2 ** 20 // 16 and 4 * math.pi * q / 2 ** 20 == pytest.approx(math.pi / 4)


def test_shape_score_arguments():
    L = _lib.load()
    for a, p in ((-1, 1), (1, -1), (TOP + 1, 1), (1, TOP + 1), (-2 ** 62, 0), (2 ** 62, 2 ** 62)):
        assert _score(a, p)[0] == _lib.FC_ERR_ARG, (a, p)
    assert L.fc_shape_score(1, 1, None) == _lib.FC_ERR_ARG


def test_names_in_header_and_binding():
    names = ("fc_run_set_shapes", "fc_run_shape_series", "fc_shape_score")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flipchain.h")) as f:
        header = f.read()
    L = _lib.load()
    for name in names:
        assert name in _lib.EXPORTED and f"int {name}(" in header
        assert getattr(L, name).restype is ctypes.c_int
    assert "#define FC_ABI_VERSION 5u" in header and _lib.FC_ABI_VERSION == 5


# ---- the model against brute force ------------------------------------------------------------

def _oracle_chain(cref, k, steps):
    if k == 2:
        spec = G.grid_graph(12, 11)
        a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
        kw = dict(labels=[-1, 1], pct=0.5)
    else:
        spec = G.grid_graph(12, 12)
        a0 = spec.assignment_array(G.quadrant_plan(spec.nodes, 6), [0, 1, 2, 3])
        kw = dict(labels=[0, 1, 2, 3], pct=0.5, proposal=_lib.FC_PROPOSE_PAIR)
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, kw.pop("pct"))
    r = cref.run(spec, a0, base=1.0, pop_lo=lo, pop_hi=hi, seed=11, chain_id=0, n_steps=steps, k=k,
                 log1mp=G.log1mp_table(spec.n, k), trace_cap=64 * steps, **kw)
    return spec, a0, events_from_trace(r["trace"]), r["final"]


def _random_shapes(spec, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 6, spec.n), rng.integers(0, 4, spec.n_edges), rng.integers(0, 3, spec.n))


@pytest.mark.parametrize("k", [2, 4])
def test_model_against_brute_force(cref, k):
    steps = 1200
    spec, a0, ev, final = _oracle_chain(cref, k, steps)
    assert len(ev) > 200
    uv = spec.edges()
    unit = G.unit_square_shapes(spec)
    for area, edge_len, ext in (unit, _random_shapes(spec, 8)):
        for t0 in (0, 500):  # the whole run, and a window that starts mid-run
            a_start = a0.astype(np.int64).copy()
            for t, v, _, _, tg in ev[ev[:, 0] <= t0]:
                a_start[v] = tg
            w = ev[ev[:, 0] > t0]
            # the window's Q range by a first pass without edges, then edges inside and around it
            m0 = SM.replay(a_start, w[:, 0], w[:, 1], w[:, 4], t0, steps, uv, area, ext, edge_len, [], k)
            edges = SM.spanning_edges([m0["q_range"]])
            m = SM.replay(a_start, w[:, 0], w[:, 1], w[:, 4], t0, steps, uv, area, ext, edge_len, edges, k)
            assert m["yields"] == steps - t0 + 1
            # brute force: every yield's assignment, and A, P, Q edge by edge in Python integers
            perim_sum, pp_sum, pp_min_sum = [0] * k, [0] * k, 0
            pp_hist = np.zeros((k, edges.size + 1), dtype=np.int64)
            pp_min_hist = np.zeros(edges.size + 1, dtype=np.int64)
            a = a0.astype(np.int64).copy()
            nxt = 0
            for t in range(steps + 1):
                while nxt < len(ev) and ev[nxt, 0] <= t:
                    a[ev[nxt, 1]] = ev[nxt, 4]
                    nxt += 1
                if t < t0:
                    continue
                A, P = [0] * k, [0] * k
                for u in range(spec.n):
                    A[a[u]] += int(area[u])
                    P[a[u]] += int(ext[u])
                for e, (u, x) in enumerate(uv):
                    if a[u] != a[x]:
                        P[a[u]] += int(edge_len[e])
                        P[a[x]] += int(edge_len[e])
                Q = [min(2 ** 20 * A[d] // P[d] ** 2, TOP) if P[d] else 0 for d in range(k)]
                for d in range(k):
                    perim_sum[d] += P[d]
                    pp_sum[d] += Q[d]
                    pp_hist[d, sum(1 for x in edges if x <= Q[d])] += 1
                pp_min_sum += min(Q)
                pp_min_hist[sum(1 for x in edges if x <= min(Q))] += 1
            assert np.array_equal(a, final) and np.array_equal(m["final"], final)
            assert list(m["area_now"]) == A and list(m["perim_now"]) == P and list(m["pp_now"]) == Q
            assert list(m["perim_sum"]) == perim_sum and list(m["pp_sum"]) == pp_sum
            assert m["pp_min_sum"] == pp_min_sum
            assert np.array_equal(m["pp_hist"], pp_hist) and np.array_equal(m["pp_min_hist"], pp_min_hist)
            assert (m["pp_hist"].sum(axis=1) == m["yields"]).all() and m["pp_min_hist"].sum() == m["yields"]
            assert (m["pp_hist"] > 0).sum(axis=1).max() >= 2  # the edges do split the Q range
        assert m0["chunk_repeats"] > 0 and m0["chunk_neighbours"] > 0


# ---- host updater and the unit-square geometry -------------------------------------------------

def test_unit_square_shapes(sec11):
    spec = G.grid_graph(5, 4)
    area, edge_len, ext = G.unit_square_shapes(spec)
    assert area.dtype == edge_len.dtype == ext.dtype == np.int32
    assert area.tolist() == [1] * 20 and edge_len.tolist() == [1] * spec.n_edges
    assert int(ext.sum()) == 2 * (5 + 4) and ext.min() == 0 and ext.max() == 2
    # one district: its perimeter is the rectangle's
    A, P = SM.areas_perims(np.zeros(20, dtype=np.int64), spec.edges()[:, 0], spec.edges()[:, 1], area, ext, edge_len, 1)
    assert (int(A[0]), int(P[0])) == (20, 18)
    assert len(G.unit_square_shapes(sec11)[1]) == sec11.n_edges
    with pytest.raises(ValueError):
        G.unit_square_shapes(G.triangular_graph(4, 4))


def test_compactness_updater():
    g = nx.grid_graph([4, 3])
    for nd in g.nodes:
        deg = g.degree[nd]
        g.nodes[nd].update(population=1, area=2)
        if deg < 4:
            g.nodes[nd]["boundary_perim"] = 4 - deg  # interior nodes carry none, as in gerrychain
    for e in g.edges:
        g.edges[e]["shared_perim"] = 1
    plan = {nd: (1 if nd[0] >= 2 else -1) for nd in g.nodes}
    part = Partition(g, plan, {"shape": Compactness()})
    out = part["shape"]
    n_side = {lab: sum(1 for nd in g.nodes if plan[nd] == lab) for lab in (-1, 1)}
    for lab in (-1, 1):
        ext = sum(g.nodes[nd].get("boundary_perim", 0) for nd in g.nodes if plan[nd] == lab)
        cut = sum(1 for u, w in g.edges if plan[u] != plan[w])
        r = out[lab]
        assert r["area"] == 2 * n_side[lab] and r["perimeter"] == ext + cut
        assert r["q"] == _rule(r["area"], r["perimeter"]) == _score(r["area"], r["perimeter"])[1]
        assert r["polsby_popper"] == pytest.approx(4 * math.pi * r["area"] / r["perimeter"] ** 2)
        assert abs(4 * math.pi * r["q"] / 2 ** 20 - r["polsby_popper"]) <= 4 * math.pi / 2 ** 20
    # a flipped partition re-evaluates
    flipped = [nd for nd in g.nodes if plan[nd] == 1 and any(plan[w] == -1 for w in g.neighbors(nd))][0]
    child = part.flip({flipped: -1})
    assert child["shape"][-1]["area"] == out[-1]["area"] + 2 and child["shape"][1]["area"] == out[1]["area"] - 2
    # the arrays the chain hands to the device, in canonical order
    spec = G.from_networkx(g)
    area, lens, ext = Compactness().arrays(g, spec, spec.edges())
    assert area.tolist() == [2] * spec.n and lens.tolist() == [1] * spec.n_edges
    assert ext.tolist() == [4 - g.degree[nd] for nd in spec.nodes]
    g.edges[(0, 0), (0, 1)]["shared_perim"] = 0.5
    with pytest.raises(ValueError):
        Compactness().arrays(g, spec, spec.edges())
