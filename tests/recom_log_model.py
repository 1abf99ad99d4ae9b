"""Host model of the series read-outs of a logged ReCom run (DESIGN.md "ReCom move log";
include/flipchain.h), computed from the **list of per-yield states** and nothing else: no event,
no replay, no segment.  Every output of the election, compactness and locality-splits series, the
plan samples and the |cut| lag sums is evaluated by the definition at every yield of the window,
one yield after the other, and summed in Python integers.  The existing event-based models
(election_model, shape_model, split_model, plans_model) assert strictly increasing event times
and cannot take a ReCom burst; tests/test_recom_log.py checks this model against them on a flip
trajectory, tests/test_recom_log_gpu.py checks the device against it.

The states come from the oracle without its trace: ``recom_run`` has no start offset, but its
random stream is counter-based, so the state at yield t of chain c is the final state of an
oracle run of t steps (``states``; yield 0 is the start plan).

The expected log (``expected_log``) is also read off the states: at each yield, the nodes whose
district differs from the yield before, ascending, with their new district and the new state's
|cut| and |B|.
"""
import numpy as np

from flipcomplexityempirical_amd import graphs as G

QMAX = 2 ** 31 - 1
XTOP = 1023
CHUNK = 64  # the replays read the log in chunks of this many events

_STATES = {}  # (case name, chain) -> (states, full oracle run): computed once, shared, not changed


def states(case, c):
    """``(S, full)``: S[t] the assignment [n] (int64) of chain c of a recom_cases.Case at yield t,
    t = 0 .. case.steps, each from an oracle run of its own; ``full`` the oracle's run of all the
    steps (its trace tells accepted from rejected steps).  Cached per (case, chain); read-only."""
    key = (case.name, c)
    if key not in _STATES:
        S = [np.asarray(case.plan(c), dtype=np.int64)]
        for t in range(1, case.steps + 1):
            r = case.oracle(c, n_steps=t)
            assert r["stats"]["steps"] == t and r["stats"]["stuck"] == 0, (case.name, c, t)
            S.append(np.asarray(r["final"], dtype=np.int64))
        full = case.oracle(c)
        assert np.array_equal(full["final"], S[-1])
        for a in S:
            a.setflags(write=False)
        _STATES[key] = (S, full)
    return _STATES[key]


def valid_flags(full):
    """flags of the valid steps of an oracle run, in yield order: entry t - 1 made yield t
    (1: rejected, 3: accepted)."""
    f = np.asarray(full["trace"]["flags"])
    return f[(f & 1) != 0]


def cut_nb(spec, S):
    """|cut| and |B| of every state (``graphs.cut_and_boundary``)."""
    cb = [G.cut_and_boundary(spec, a) for a in S]
    return [c for c, _, _ in cb], [b for _, b, _ in cb]


def expected_log(S, t0, cut, nb):
    """The log of the window whose yields t0 .. t0 + len(S) - 1 have the states S: rows
    (t, v, target, cut, nb), and the per-yield burst lengths [len(S)] (entry 0 is 0)."""
    rows, lens = [], [0]
    for i in range(1, len(S)):
        moved = np.nonzero(S[i] != S[i - 1])[0]
        lens.append(int(moved.size))
        rows += [(t0 + i, int(v), int(S[i][v]), cut[i], nb[i]) for v in moved]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 5), np.asarray(lens, dtype=np.int64)


def straddles(lens, chunk=CHUNK):
    """Bursts that lie across a multiple of ``chunk`` in the log index (events lo .. hi - 1 with a
    multiple m of chunk, lo < m < hi)."""
    hi = np.cumsum(lens)
    lo = hi - lens
    return int(np.sum((lens > 1) & ((hi - 1) // chunk > lo // chunk)))


def _hist(values, edges):
    """values' counts by the number of edges <= value (searchsorted side="right")."""
    h = [0] * (len(edges) + 1)
    for x in values:
        h[sum(1 for e in edges if e <= x)] += 1
    return np.asarray(h, dtype=np.int64)


def elections(S, cols, elections, edges, k):
    """fc_run_election_series of one chain whose window's yields have the states S."""
    cols = np.asarray(cols, dtype=np.int64)
    n_cols, n_el = cols.shape[1], len(elections)
    edges = [int(e) for e in np.asarray(edges).reshape(-1)]
    tally_sum = np.zeros((k, n_cols), dtype=np.int64)
    seats_hist = np.zeros((n_el, k + 1), dtype=np.int64)
    wins_sum = np.zeros((n_el, k), dtype=np.int64)
    gap_sum = [0] * n_el
    gaps = [[] for _ in range(n_el)]
    for a in S:
        T = np.asarray([[int(cols[a == d, j].sum()) for j in range(n_cols)] for d in range(k)], dtype=np.int64)
        tally_sum += T
        for e, (ca, cb) in enumerate(elections):
            seats, gap = 0, 0
            for d in range(k):
                x, y = int(T[d, ca]), int(T[d, cb])
                if x > y:
                    seats += 1
                    wins_sum[e, d] += 1
                    gap += 3 * y - x
                elif x < y:
                    gap += y - 3 * x
            seats_hist[e, seats] += 1
            gap_sum[e] += gap
            gaps[e].append(gap)
    out = {"yields": len(S), "tally_now": T, "tally_sum": tally_sum, "seats_hist": seats_hist, "wins_sum": wins_sum,
           "gap_sum": np.asarray(gap_sum, dtype=np.int64),
           "gap_hist": np.stack([_hist(g, edges) for g in gaps]) if n_el else np.zeros((0, len(edges) + 1), np.int64),
           "gap_range": [(min(g), max(g)) for g in gaps]}
    return out


def shapes(S, edges_uv, area, ext, edge_len, pp_edges, k):
    """fc_run_shape_series of one chain whose window's yields have the states S."""
    uv = np.asarray(edges_uv, dtype=np.int64).reshape(-1, 2)
    n = S[0].size
    area = [int(x) for x in area]
    ext = [0] * n if ext is None else [int(x) for x in ext]
    edge_len = [int(x) for x in edge_len]
    pp_edges = [int(e) for e in np.asarray(pp_edges).reshape(-1)]
    perim_sum, pp_sum, pp_min_sum = [0] * k, [0] * k, 0
    Qs, Qmins = [], []
    for a in S:
        A, P = [0] * k, [0] * k
        for u in range(n):
            A[a[u]] += area[u]
            P[a[u]] += ext[u]
        for e, (u, w) in enumerate(uv):
            if a[u] != a[w]:
                P[a[u]] += edge_len[e]
                P[a[w]] += edge_len[e]
        Q = [min((A[d] << 20) // (P[d] * P[d]), QMAX) if P[d] else 0 for d in range(k)]
        for d in range(k):
            perim_sum[d] += P[d]
            pp_sum[d] += Q[d]
        pp_min_sum += min(Q)
        Qs.append(Q)
        Qmins.append(min(Q))
    i64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return {"yields": len(S), "area_now": i64(A), "perim_now": i64(P), "pp_now": i64(Q), "perim_sum": i64(perim_sum),
            "pp_sum": i64(pp_sum), "pp_min_sum": pp_min_sum,
            "pp_hist": np.stack([_hist([q[d] for q in Qs], pp_edges) for d in range(k)]),
            "pp_min_hist": _hist(Qmins, pp_edges), "q_range": (min(map(min, Qs)), max(map(max, Qs)))}


def splits(S, node_loc, k):
    """fc_run_split_series of one chain whose window's yields have the states S, and what
    ``FlipRun.split_series`` derives from ``cells_now``."""
    node_loc = np.asarray(node_loc, dtype=np.int64)
    n_loc = int(node_loc.max()) + 1
    sizes = np.bincount(node_loc, minlength=n_loc)
    x_max = int(np.minimum(sizes, k).sum()) - n_loc
    X = min(x_max, XTOP)
    split_sum, parts_sum = np.zeros(n_loc, dtype=np.int64), np.zeros(n_loc, dtype=np.int64)
    dlocs_sum = np.zeros(k, dtype=np.int64)
    splits_hist, excess_hist = np.zeros(n_loc + 1, dtype=np.int64), np.zeros(X + 1, dtype=np.int64)
    sq_sum = 0
    for a in S:
        cells = np.zeros((n_loc, k), dtype=np.int64)
        for u in range(a.size):
            cells[node_loc[u], a[u]] += 1
        parts = (cells > 0).sum(axis=1)
        dlocs = (cells > 0).sum(axis=0)
        n_split, excess, sq = int((parts >= 2).sum()), int((parts - 1).sum()), int((cells * cells).sum())
        split_sum += parts >= 2
        parts_sum += parts
        dlocs_sum += dlocs
        sq_sum += sq
        splits_hist[n_split] += 1
        excess_hist[min(excess, X)] += 1
    return {"yields": len(S), "x_max": x_max, "cells_now": cells, "split_sum": split_sum, "parts_sum": parts_sum,
            "dlocs_sum": dlocs_sum, "sq_sum": sq_sum, "splits_hist": splits_hist, "excess_hist": excess_hist,
            "parts_now": parts, "splits_now": n_split, "excess_now": excess, "sq_now": sq, "dlocs_now": dlocs}


def plans(S, t0, cut, nb, pop, times, k):
    """fc_run_sample_plans of one chain whose window's yields t0 .. have the states S (``cut`` /
    ``nb``: per state), at the absolute yields ``times``."""
    pop = np.asarray(pop, dtype=np.int64)
    idx = [int(t) - t0 for t in times]
    assert all(0 <= i < len(S) for i in idx)
    m = len(idx)
    return {"plans": np.asarray([S[i] for i in idx], dtype=np.int8).reshape(m, S[0].size),
            "cut": np.asarray([cut[i] for i in idx], dtype=np.int64),
            "nb": np.asarray([nb[i] for i in idx], dtype=np.int64),
            "dist0": np.asarray([int((S[i] != S[0]).sum()) for i in idx], dtype=np.int64),
            "pops": np.asarray([[int(pop[S[i] == d].sum()) for d in range(k)] for i in idx],
                               dtype=np.int64).reshape(m, k)}


def lag_sums(cut, lags):
    """sum_t x_t x_{t + L} over the window's |cut| series, exact."""
    x = [int(v) for v in cut]
    return np.asarray([sum(x[t] * x[t + L] for t in range(len(x) - L)) if L < len(x) else 0 for L in lags],
                      dtype=np.int64)
