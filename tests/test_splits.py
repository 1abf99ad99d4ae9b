"""Locality-splits series, the parts that need no GPU: ``fc_splits_eval`` (the rule
the device applies per flip) against Python integers; the host model (tests/split_model.py) against
a brute-force recomputation of every yield of an oracle chain, with the invariants that tie the
outputs together; the new names in the header and the binding; ``block_localities`` and the
host-side ``LocalitySplits`` updater."""
import ctypes
import os

import networkx as nx
import numpy as np
import pytest

import split_model as SM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.chain import LocalitySplits, Partition
from oracle.flipref import events_from_trace

I64 = ctypes.POINTER(ctypes.c_int64)


def _oracle_chain(cref, k, steps):
    """The oracle chains of tests/test_shapes.py: 12 x 11 grid, k = 2; 12 x 12 grid, k = 4."""
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


def _eval(cells, n_loc=None, k=None):
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    n_loc = cells.shape[0] if n_loc is None else n_loc
    k = cells.shape[1] if k is None else k
    out = [ctypes.c_int64(-7) for _ in range(3)]
    rc = _lib.load().fc_splits_eval(n_loc, k, cells.ctypes.data_as(I64), *(ctypes.byref(x) for x in out))
    return (rc,) + tuple(int(x.value) for x in out)


def _rule(cells):
    """The issue's definitions, in Python integers."""
    rows = [[int(x) for x in row] for row in cells]
    parts = [sum(1 for x in row if x > 0) for row in rows]
    return (sum(1 for p in parts if p >= 2), sum(p - 1 for p in parts), sum(x * x for row in rows for x in row))


def test_splits_eval_against_python_integers():
    rng = np.random.default_rng(5)
    cases = [np.array([[7]]),                                   # one district, one locality
             np.array([[3], [1], [65535]]),                     # one district
             np.eye(6, dtype=np.int64),                         # every node its own locality, k = 6
             np.array([[5, 0, 9, 1]]),                          # one locality
             np.array([[65535, 65535], [65535, 0], [0, 1]]),    # counts of 65,535
             np.array([[0, 0, 1], [1, 1, 1], [2, 0, 0]])]
    for k in range(1, 33):
        cells = rng.integers(0, 4, (5, k))
        cells[np.arange(5), rng.integers(0, k, 5)] += 1  # no empty locality
        cases.append(cells)
        cases.append(np.ones((2, k), dtype=np.int64))   # every cell occupied: excess k - 1 each
        one = np.zeros((3, k), dtype=np.int64)
        one[:, k - 1] = [1, 65535, 2]                     # nothing split, whatever k
        cases.append(one)
    for cells in cases:
        rc, s, x, q = _eval(cells)
        assert rc == _lib.FC_OK and (s, x, q) == _rule(cells), (cells, s, x, q)
        a = SM.aggregates(np.asarray(cells, dtype=np.int64))
        assert (s, x, q) == (a[1], a[2], a[3])
    assert _eval(np.array([[65535, 65535]]))[1:] == (1, 1, 2 * 65535 ** 2)
    # any output may be NULL
    cells = np.ascontiguousarray([[1, 2]], dtype=np.int64)
    assert _lib.load().fc_splits_eval(1, 2, cells.ctypes.data_as(I64), None, None, None) == _lib.FC_OK


def test_splits_eval_arguments():
    L = _lib.load()
    ok = np.array([[1, 2], [3, 0]])
    assert _eval(ok)[0] == _lib.FC_OK
    assert L.fc_splits_eval(2, 2, None, None, None, None) == _lib.FC_ERR_ARG
    for n_loc, k in ((0, 2), (-1, 2), (2, 0), (2, 33)):
        assert _eval(np.ones((4, 40)), n_loc, k)[0] == _lib.FC_ERR_ARG, (n_loc, k)
    for bad in ([[1, -1], [3, 0]], [[1, 65536], [3, 0]], [[1, 2], [0, 0]]):  # the last: an empty locality
        assert _eval(np.array(bad))[0] == _lib.FC_ERR_ARG, bad
    assert b"fc_splits_eval" in L.fc_last_error()


def test_names_in_header_and_binding():
    names = ("fc_run_set_localities", "fc_run_split_series", "fc_splits_eval")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flipchain.h")) as f:
        header = f.read()
    L = _lib.load()
    for name in names:
        assert name in _lib.EXPORTED and f"int {name}(" in header
        assert getattr(L, name).restype is ctypes.c_int
    assert "#define FC_ABI_VERSION 5u" in header and _lib.FC_ABI_VERSION == 5


# ---- the model against brute force ------------------------------------------------------------

def _labellings(spec, k):
    blocks = G.block_localities(spec, 2, 3) if k == 2 else G.block_localities(spec, 3, 3)
    return {"blocks": blocks, "columns": G.block_localities(spec, 1, 12), "one": np.zeros(spec.n, dtype=np.int32),
            "nodes": np.arange(spec.n, dtype=np.int32)}


@pytest.mark.parametrize("k", [2, 4])
def test_model_against_brute_force(cref, k):
    steps = 1200
    spec, a0, ev, final = _oracle_chain(cref, k, steps)
    assert len(ev) > 200
    for name, node_loc in _labellings(spec, k).items():
        n_loc = int(node_loc.max()) + 1
        x_max = SM.x_max_of(node_loc, n_loc, k)
        for t0 in (0, 500):  # the whole run, and a window that starts mid-run
            a_start = a0.astype(np.int64).copy()
            for t, v, _, _, tg in ev[ev[:, 0] <= t0]:
                a_start[v] = tg
            w = ev[ev[:, 0] > t0]
            m = SM.replay(a_start, w[:, 0], w[:, 1], w[:, 4], t0, steps, node_loc, k)
            assert m["yields"] == steps - t0 + 1 and m["x_max"] == x_max
            # brute force: every yield's assignment and its table, node by node in Python integers
            split_sum, parts_sum, dlocs_sum, sq_sum = [0] * n_loc, [0] * n_loc, [0] * k, 0
            splits_hist, excess_hist = [0] * (n_loc + 1), [0] * (min(x_max, 1023) + 1)
            a = a0.astype(np.int64).copy()
            nxt = 0
            for t in range(steps + 1):
                while nxt < len(ev) and ev[nxt, 0] <= t:
                    a[ev[nxt, 1]] = ev[nxt, 4]
                    nxt += 1
                if t < t0:
                    continue
                cells = [[0] * k for _ in range(n_loc)]
                for u in range(spec.n):
                    cells[node_loc[u]][a[u]] += 1
                parts = [sum(1 for x in row if x > 0) for row in cells]
                for c in range(n_loc):
                    split_sum[c] += parts[c] >= 2
                    parts_sum[c] += parts[c]
                for d in range(k):
                    dlocs_sum[d] += sum(1 for c in range(n_loc) if cells[c][d] > 0)
                sq_sum += sum(x * x for row in cells for x in row)
                splits_hist[sum(1 for p in parts if p >= 2)] += 1
                excess_hist[min(sum(p - 1 for p in parts), min(x_max, 1023))] += 1
            assert np.array_equal(a, final) and np.array_equal(m["final"], final)
            assert m["cells_now"].tolist() == cells and m["parts_now"].tolist() == parts
            assert m["split_sum"].tolist() == split_sum and m["parts_sum"].tolist() == parts_sum
            assert m["dlocs_sum"].tolist() == dlocs_sum and m["sq_sum"] == sq_sum
            assert m["splits_hist"].tolist() == splits_hist and m["excess_hist"].tolist() == excess_hist
            assert (m["splits_now"], m["excess_now"], m["sq_now"]) == _rule(cells)
            SM.check_invariants(m, n_loc, spec.n, pops=np.bincount(final, minlength=k))
        if name == "blocks":
            assert m["crossings"] > 0 and m["chunk_same_loc"] > 0
            assert (m["splits_hist"] > 0).sum() >= 2 and (m["excess_hist"] > 0).sum() >= 2
        if name == "nodes":
            assert m["crossings"] == 2 * len(w) and x_max == 0 and m["excess_hist"].tolist() == [m["yields"]]


# ---- block_localities and the host updater ------------------------------------------------------

def test_block_localities(sec11):
    spec = G.grid_graph(12, 11)
    loc = G.block_localities(spec, 2, 3)
    assert loc.dtype == np.int32 and loc.shape == (132,) and int(loc.max()) + 1 == 24
    # (grid_graph(12, 11) has x = 0..10 and y = 0..11: the last column of blocks is one cell wide)
    assert np.bincount(loc).tolist() == [6] * 20 + [3] * 4
    by_block = {}
    for nd, c in zip(spec.nodes, loc):
        by_block.setdefault((nd[0] // 2, nd[1] // 3), set()).add(int(c))
    assert all(len(x) == 1 for x in by_block.values())
    assert [by_block[b].copy().pop() for b in sorted(by_block)] == list(range(24))  # ascending block order
    # a threshold plan at x = 6 runs along block borders: no locality split at the start
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    assert SM.aggregates(SM.cell_table(a0, loc, 24, 2))[1] == 0
    assert int(G.block_localities(spec, 1, 12).max()) + 1 == 11  # columns
    assert int(G.block_localities(spec, 1, 11).max()) + 1 == 22  # columns cut once at y = 11
    assert G.block_localities(spec, 11, 12).tolist() == [0] * 132
    # sec11 lacks its four corner nodes: the blocks that remain are numbered densely
    loc = G.block_localities(sec11, 1, 1)
    assert np.array_equal(loc, np.arange(sec11.n))
    assert int(G.block_localities(sec11, 4, 4).max()) + 1 == 100
    for bad in ((0, 1), (1, 0), (1.5, 1)):
        with pytest.raises(ValueError):
            G.block_localities(spec, *bad)
    with pytest.raises(ValueError):
        G.block_localities(G.from_networkx(nx.path_graph(4)), 1, 1)


def test_locality_splits_updater():
    g = nx.grid_graph([4, 3])  # nodes (x, y): x 0..2, y 0..3
    for nd in g.nodes:
        g.nodes[nd].update(population=1, county="west" if nd[1] < 2 else "east")
    plan = {nd: (1 if nd[1] >= 2 else -1) for nd in g.nodes}
    part = Partition(g, plan, {"splits": LocalitySplits()})
    out = part["splits"]
    assert out["west"] == {"parts": 1, "split": False, "districts": [-1]}
    assert out["east"] == {"parts": 1, "split": False, "districts": [1]}
    assert out["num_split"] == 0 and out["excess"] == 0
    # a flipped child partition re-evaluates
    child = part.flip({(0, 2): -1})
    out = child["splits"]
    assert out["east"] == {"parts": 2, "split": True, "districts": [-1, 1]} and out["west"]["parts"] == 1
    assert out["num_split"] == 1 and out["excess"] == 1
    # the arrays the chain hands to the device, in canonical order; they agree with the model
    spec = G.from_networkx(g)
    labels, node_loc = LocalitySplits().arrays(g, spec)
    assert labels == ["east", "west"] and node_loc.dtype == np.int32
    assert node_loc.tolist() == [0 if nd[1] >= 2 else 1 for nd in spec.nodes]
    a = spec.assignment_array(dict(child.assignment.items()), [-1, 1])
    parts, splits, excess, _, _ = SM.aggregates(SM.cell_table(a, node_loc, 2, 2))
    assert parts.tolist() == [2, 1] and (splits, excess) == (1, 1)
    # another attribute name, and a node without it
    for nd in g.nodes:
        g.nodes[nd]["muni"] = nd[0]
    assert Partition(g, plan, {"m": LocalitySplits("muni")})["m"]["num_split"] == 3
    del g.nodes[(1, 1)]["muni"]
    with pytest.raises(ValueError):
        LocalitySplits("muni").arrays(g, spec)
    with pytest.raises(ValueError):
        Partition(g, plan, {"m": LocalitySplits("muni")})["m"]
