"""Host model of the locality-splits series (include/flipchain.h): a plain numpy /
Python-integer replay of one chain's accepted-flip log against a node labelling.  It shares no code
with the device path and does not call ``fc_splits_eval``; tests/test_splits.py checks it against a
brute-force recomputation of every yield, tests/test_splits_gpu.py checks the device against it.

Every per-yield quantity is a per-segment value (a segment: the yields between two accepted flips)
expanded by the segment's run length (``np.repeat``) or weighted by it.  The cell table of every
segment is recomputed from that segment's assignment by the definition, not by the device's
incremental rule.
"""
import numpy as np

CHUNK = 64  # the device reads its log in chunks of this many events
XTOP = 1023  # excess_hist's top bin


def cell_table(a, node_loc, n_loc, k):
    """cells[n_loc, k] of the assignment ``a`` [n] from the definition."""
    cells = np.zeros((n_loc, k), dtype=np.int64)
    np.add.at(cells, (node_loc, a), 1)
    return cells


def aggregates(cells):
    """parts [n_loc], splits, excess, sq, dlocs [k] of one table."""
    occ = cells > 0
    parts = occ.sum(axis=1)
    return parts, int((parts >= 2).sum()), int((parts - 1).sum()), int((cells * cells).sum()), occ.sum(axis=0)


def x_max_of(node_loc, n_loc, k):
    return int(np.minimum(np.bincount(node_loc, minlength=n_loc), k).sum()) - n_loc


def replay(a0, ev_t, ev_v, ev_target, t0, T, node_loc, k):
    """``a0`` [n] district ids at yield ``t0``; events ``(ev_t, ev_v, ev_target)`` in log order,
    event i making ``a[ev_v[i]] = ev_target[i]`` from yield ``ev_t[i]`` on; window yields
    ``t0 .. T``; ``node_loc`` [n] labels ``0 .. n_loc - 1``.  Returns the outputs of
    ``fc_run_split_series`` for this chain and those ``FlipRun.split_series`` derives, plus
    ``yields``, ``final`` (the assignment at yield T), ``crossings`` (a cell reaching or leaving 0)
    and ``chunk_same_loc`` (events whose locality an earlier event of the same chunk of 64 touched;
    chunks counted from the window's first event)."""
    a = np.asarray(a0, dtype=np.int64).copy()
    node_loc = np.asarray(node_loc, dtype=np.int64)
    n_loc = int(node_loc.max()) + 1
    ev_t = np.asarray(ev_t, dtype=np.int64)
    ev_v = np.asarray(ev_v, dtype=np.int64)
    ev_target = np.asarray(ev_target, dtype=np.int64)
    m = ev_t.size
    assert ev_v.size == m and ev_target.size == m
    if m:
        assert ev_t[0] > t0 and ev_t[-1] <= T and (np.diff(ev_t) > 0).all()
    runs = np.diff(np.concatenate([[t0], ev_t, [T + 1]]))  # yields of each of the m + 1 segments
    parts = np.zeros((m + 1, n_loc), dtype=np.int64)
    dlocs = np.zeros((m + 1, k), dtype=np.int64)
    splits = np.zeros(m + 1, dtype=np.int64)
    excess = np.zeros(m + 1, dtype=np.int64)
    sq = np.zeros(m + 1, dtype=np.int64)
    cells = cell_table(a, node_loc, n_loc, k)
    parts[0], splits[0], excess[0], sq[0], dlocs[0] = aggregates(cells)
    crossings = 0
    for i in range(m):
        assert a[ev_v[i]] != ev_target[i]
        a[ev_v[i]] = ev_target[i]
        new = cell_table(a, node_loc, n_loc, k)
        crossings += int(((new > 0) != (cells > 0)).sum())
        cells = new
        parts[i + 1], splits[i + 1], excess[i + 1], sq[i + 1], dlocs[i + 1] = aggregates(cells)
    x_max = x_max_of(node_loc, n_loc, k)
    X = min(x_max, XTOP)
    assert excess.max() <= x_max and parts.min() >= 1
    same = 0
    for lo in range(0, m, CHUNK):
        seen = set()
        for v in ev_v[lo:lo + CHUNK]:
            c = int(node_loc[v])
            same += c in seen
            seen.add(c)
    return {"yields": int(runs.sum()), "final": a, "x_max": x_max, "cells_now": cells,
            "split_sum": ((parts >= 2) * runs[:, None]).sum(axis=0), "parts_sum": (parts * runs[:, None]).sum(axis=0),
            "dlocs_sum": (dlocs * runs[:, None]).sum(axis=0), "sq_sum": int((sq * runs).sum()),
            "splits_hist": np.bincount(np.repeat(splits, runs), minlength=n_loc + 1),
            "excess_hist": np.bincount(np.repeat(np.minimum(excess, X), runs), minlength=X + 1),
            "parts_now": parts[-1].copy(), "splits_now": int(splits[-1]), "excess_now": int(excess[-1]),
            "sq_now": int(sq[-1]), "dlocs_now": dlocs[-1].copy(), "splits_values": np.unique(splits),
            "crossings": crossings, "chunk_same_loc": same}


def replay_run(run, c, node_loc, a0):
    """The model fed with chain ``c`` of a FlipRun: its event log, ``stats()`` and the window-start
    assignment ``a0`` [n] (the initial state, or ``run.state()[c]`` read at the last reset)."""
    st = run.stats()
    ev = run.events(c)
    return replay(a0, ev["t"], ev["v"], ev["target"], int(st["series_t0"][c]), int(st["steps"][c]), node_loc,
                  run.cfg.k)


ARRAYS = ("cells_now", "split_sum", "parts_sum", "dlocs_sum", "splits_hist", "excess_hist", "parts_now", "dlocs_now")
SCALARS = ("sq_sum", "splits_now", "excess_now", "sq_now")


def check_invariants(r, n_loc, n, pops=None):
    """The relations between the outputs of one chain (``r``: the model's dict, or one chain's
    entries of a ``split_series`` result)."""
    y = int(r["yields"])
    sh, eh = np.asarray(r["splits_hist"]), np.asarray(r["excess_hist"])
    assert int(sh.sum()) == y and int(eh.sum()) == y
    assert int(np.sum(r["split_sum"])) == int((np.arange(sh.size) * sh).sum())
    assert int(np.sum(r["parts_sum"])) == int(np.sum(r["dlocs_sum"]))
    if int(r["x_max"]) <= XTOP:
        assert int(np.sum(r["parts_sum"])) - n_loc * y == int((np.arange(eh.size) * eh).sum())
    assert int(np.sum(r["cells_now"])) == n
    if pops is not None:  # unit populations
        assert np.array_equal(np.asarray(r["cells_now"]).sum(axis=0), pops)
    if n_loc == n:  # one node per locality: nothing can be split
        assert int(sh[0]) == y and int(r["sq_sum"]) == n * y


def assert_matches(got, i, exp):
    """Entry ``i`` of a ``FlipRun.split_series`` result equals the model's ``exp``, bit for bit."""
    assert int(got["yields"][i]) == exp["yields"] and got["x_max"] == exp["x_max"]
    for key in ARRAYS:
        assert got[key][i].shape == np.asarray(exp[key]).shape, (key, got[key][i].shape)
        assert np.array_equal(got[key][i], exp[key]), (key, got[key][i], exp[key])
    for key in SCALARS:
        assert int(got[key][i]) == exp[key], (key, int(got[key][i]), exp[key])
