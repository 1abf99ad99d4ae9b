"""Host model of the compactness series (include/flipchain.h): a plain numpy /
Python-integer replay of one chain's accepted-flip log against node areas, exterior lengths and
shared edge lengths.  It shares no code with the device path and does not call ``fc_shape_score``;
tests/test_shapes.py checks it against a brute-force recomputation of every yield,
tests/test_shapes_gpu.py checks the device against it.

Every per-yield quantity is a per-segment value (a segment: the yields between two accepted flips)
expanded by the segment's run length (``np.repeat``) or weighted by it.  The perimeters of every
segment are recomputed from the definition (a sum over the cut edges of that segment's
assignment), not by the device's incremental rule.
"""
import numpy as np

CHUNK = 64  # the device reads its log in chunks of this many events
QMAX = 2 ** 31 - 1


def score(area, perim):
    """Q of the definition, in Python integers."""
    area, perim = int(area), int(perim)
    return min((area << 20) // (perim * perim), QMAX) if perim else 0


def areas_perims(a, eu, ev, area, ext, edge_len, k):
    """A[k], P[k] of the assignment ``a`` [n] from the definition."""
    A = np.bincount(a, weights=None if area is None else area, minlength=k).astype(np.int64)
    P = np.bincount(a, weights=ext, minlength=k).astype(np.int64)
    cut = a[eu] != a[ev]
    P += np.bincount(a[eu][cut], weights=edge_len[cut], minlength=k).astype(np.int64)
    P += np.bincount(a[ev][cut], weights=edge_len[cut], minlength=k).astype(np.int64)
    return A, P


def replay(a0, ev_t, ev_v, ev_target, t0, T, edges_uv, area, ext, edge_len, pp_edges, k):
    """``a0`` [n] district ids at yield ``t0``; events ``(ev_t, ev_v, ev_target)`` in log order,
    event i making ``a[ev_v[i]] = ev_target[i]`` from yield ``ev_t[i]`` on; window yields
    ``t0 .. T``; ``edges_uv`` [E, 2] the canonical edges; ``area`` / ``ext`` [n] (``ext`` None: 0),
    ``edge_len`` [E]; ``pp_edges`` ascending ints.  Returns the outputs of ``fc_run_shape_series``
    for this chain plus ``yields``, ``final`` (the assignment at yield T), ``chunk_repeats`` (events
    whose node occurs earlier in the same chunk of 64), ``chunk_neighbours`` (events whose node has
    a graph neighbour flipped earlier in the same chunk) and ``q_range`` (min, max of Q over
    districts and yields)."""
    a = np.asarray(a0, dtype=np.int64).copy()
    n = a.size
    uv = np.asarray(edges_uv, dtype=np.int64).reshape(-1, 2)
    eu, ev = uv[:, 0], uv[:, 1]
    area = np.asarray(area, dtype=np.int64)
    ext = np.zeros(n, dtype=np.int64) if ext is None else np.asarray(ext, dtype=np.int64)
    edge_len = np.asarray(edge_len, dtype=np.int64)
    ev_t = np.asarray(ev_t, dtype=np.int64)
    ev_v = np.asarray(ev_v, dtype=np.int64)
    ev_target = np.asarray(ev_target, dtype=np.int64)
    m = ev_t.size
    assert ev_v.size == m and ev_target.size == m
    if m:
        assert ev_t[0] > t0 and ev_t[-1] <= T and (np.diff(ev_t) > 0).all()
    runs = np.diff(np.concatenate([[t0], ev_t, [T + 1]]))  # yields of each of the m + 1 segments
    # A, P of every segment, each from the definition
    A = np.zeros((m + 1, k), dtype=np.int64)
    P = np.zeros((m + 1, k), dtype=np.int64)
    A[0], P[0] = areas_perims(a, eu, ev, area, ext, edge_len, k)
    for i in range(m):
        assert a[ev_v[i]] != ev_target[i]
        a[ev_v[i]] = ev_target[i]
        A[i + 1], P[i + 1] = areas_perims(a, eu, ev, area, ext, edge_len, k)
    Q = np.asarray([[score(A[s, d], P[s, d]) for d in range(k)] for s in range(m + 1)], dtype=np.int64)
    Qmin = Q.min(axis=1)
    pp_edges = np.asarray(pp_edges, dtype=np.int64).reshape(-1)
    nb = pp_edges.size + 1
    out = {"yields": int(runs.sum()), "final": a, "area_now": A[-1].copy(), "perim_now": P[-1].copy(),
           "pp_now": Q[-1].copy(), "perim_sum": (P * runs[:, None]).sum(axis=0),
           "pp_sum": (Q * runs[:, None]).sum(axis=0), "pp_min_sum": int((Qmin * runs).sum()),
           "pp_hist": np.zeros((k, nb), dtype=np.int64), "pp_min_hist": np.zeros(nb, dtype=np.int64),
           "q_range": (int(Q.min()), int(Q.max()))}
    if pp_edges.size:
        for d in range(k):
            out["pp_hist"][d] = np.bincount(np.searchsorted(pp_edges, np.repeat(Q[:, d], runs), side="right"),
                                            minlength=nb)
        out["pp_min_hist"] = np.bincount(np.searchsorted(pp_edges, np.repeat(Qmin, runs), side="right"), minlength=nb)
    nbrs = [set() for _ in range(n)]
    for u, w in uv:
        nbrs[u].add(int(w))
        nbrs[w].add(int(u))
    rep = nei = 0
    for lo in range(0, m, CHUNK):
        seen = set()
        for v in ev_v[lo:lo + CHUNK]:
            v = int(v)
            rep += v in seen
            nei += bool(nbrs[v] & seen)
            seen.add(v)
    out["chunk_repeats"], out["chunk_neighbours"] = rep, nei
    return out


def spanning_edges(q_ranges, per=5):
    """Histogram edges that split every Q range ``(lo, hi)``: ``per`` evenly spaced edges across
    each range (one beyond each end)."""
    pts = [np.linspace(lo - 2, hi + 2, per).astype(np.int64) for lo, hi in q_ranges]
    return np.unique(np.concatenate(pts))


def replay_run(run, c, shapes, pp_edges, a0):
    """The model fed with chain ``c`` of a FlipRun: its event log, ``stats()`` and the window-start
    assignment ``a0`` [n] (the initial state, or ``run.state()[c]`` read at the last reset);
    ``shapes`` = (area, edge_len, ext)."""
    st = run.stats()
    ev = run.events(c)
    area, edge_len, ext = shapes
    return replay(a0, ev["t"], ev["v"], ev["target"], int(st["series_t0"][c]), int(st["steps"][c]),
                  run.graph.edges(), area, ext, edge_len, pp_edges, run.cfg.k)


KEYS = ("area_now", "perim_now", "perim_sum", "pp_now", "pp_sum", "pp_min_sum")


def assert_matches(got, i, exp, with_hist=True):
    """Entry ``i`` of a ``FlipRun.shape_series`` result equals the model's ``exp``, bit for bit, and
    every histogram row sums to the window's yields."""
    assert int(got["yields"][i]) == exp["yields"]
    for key in KEYS:
        assert np.array_equal(got[key][i], exp[key]), (key, got[key][i], exp[key])
    if with_hist:
        for key in ("pp_hist", "pp_min_hist"):
            assert np.array_equal(got[key][i], exp[key]), (key, got[key][i], exp[key])
            assert (got[key][i].sum(axis=-1) == exp["yields"]).all()
