"""Host model of the election series (include/flipchain.h): a plain numpy replay of
one chain's accepted-flip log against node vote columns.  It shares no code with the device path
and does not call ``fc_election_eval``; tests/test_election.py checks it against a brute-force
recomputation of every yield, tests/test_election_gpu.py checks the device against it.

Every per-yield quantity is a per-segment value (a segment: the yields between two accepted flips)
expanded by the segment's run length (``np.repeat``) or weighted by it, in Python / int64 integers.
"""
import numpy as np

CHUNK = 64  # the device reads its log in chunks of this many events


def replay(a0, ev_t, ev_v, ev_target, t0, T, cols, elections, edges, k):
    """``a0`` [n] district ids at yield ``t0``; events ``(ev_t, ev_v, ev_target)`` in log order,
    event i making ``a[ev_v[i]] = ev_target[i]`` from yield ``ev_t[i]`` on; window yields
    ``t0 .. T``; ``cols`` [n, n_cols]; ``elections`` [(col_a, col_b)]; ``edges`` ascending ints.
    Returns the outputs of ``fc_run_election_series`` for this chain plus ``yields``, ``final``
    (the assignment at yield T), ``ties`` (yields with a tied district in some election) and
    ``chunk_repeats`` (events whose node occurs earlier in the same chunk of 64)."""
    a0 = np.asarray(a0, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    ev_t = np.asarray(ev_t, dtype=np.int64)
    ev_v = np.asarray(ev_v, dtype=np.int64)
    ev_target = np.asarray(ev_target, dtype=np.int64)
    m, n_cols = ev_t.size, cols.shape[1]
    assert ev_v.size == m and ev_target.size == m
    if m:
        assert ev_t[0] > t0 and ev_t[-1] <= T and (np.diff(ev_t) > 0).all()
    runs = np.diff(np.concatenate([[t0], ev_t, [T + 1]]))  # yields of each of the m + 1 segments
    # the district every event's node leaves
    cur = a0.copy()
    old = np.zeros(m, dtype=np.int64)
    for i in range(m):
        old[i] = cur[ev_v[i]]
        cur[ev_v[i]] = ev_target[i]
    assert (old != ev_target).all()
    # tallies of every segment: the initial ones plus the running sum of the events' moves
    S0 = np.zeros((k, n_cols), dtype=np.int64)
    np.add.at(S0, a0, cols)
    delta = np.zeros((m + 1, k, n_cols), dtype=np.int64)
    idx = np.arange(1, m + 1)
    np.add.at(delta, (idx, old), -cols[ev_v])
    np.add.at(delta, (idx, ev_target), cols[ev_v])
    S = S0[None] + np.cumsum(delta, axis=0)
    assert (S >= 0).all()
    out = {"yields": int(runs.sum()), "final": cur,
           "tally_now": S[-1].copy(), "tally_sum": (S * runs[:, None, None]).sum(axis=0)}
    n_el = len(elections)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1)
    out["seats_hist"] = np.zeros((n_el, k + 1), dtype=np.int64)
    out["wins_sum"] = np.zeros((n_el, k), dtype=np.int64)
    out["gap_sum"] = np.zeros(n_el, dtype=np.int64)
    out["gap_hist"] = np.zeros((n_el, edges.size + 1), dtype=np.int64)
    ties = np.zeros(m + 1, dtype=bool)
    for e, (ca, cb) in enumerate(elections):
        a, b = S[:, :, ca], S[:, :, cb]
        win = a > b
        ties |= (a == b).any(axis=1)
        out["seats_hist"][e] = np.bincount(np.repeat(win.sum(axis=1), runs), minlength=k + 1)
        out["wins_sum"][e] = (win * runs[:, None]).sum(axis=0)
        g = np.where(a > b, 3 * b - a, np.where(a < b, b - 3 * a, 0))
        gap = g.sum(axis=1)
        out["gap_sum"][e] = int((gap * runs).sum())
        if edges.size:
            out["gap_hist"][e] = np.bincount(np.searchsorted(edges, np.repeat(gap, runs), side="right"),
                                             minlength=edges.size + 1)
        out.setdefault("gap_range", []).append((int(gap.min()), int(gap.max())))
    out["ties"] = int(runs[ties].sum()) if n_el else 0
    rep = 0
    for lo in range(0, m, CHUNK):
        v = ev_v[lo:lo + CHUNK]
        rep += v.size - np.unique(v).size
    out["chunk_repeats"] = rep
    return out


def spanning_edges(gap_ranges, per=5):
    """Histogram edges that split every election's gap range ``(lo, hi)``: ``per`` evenly spaced
    edges across each range (one beyond each end), and 0."""
    pts = [np.linspace(lo - 2, hi + 2, per).astype(np.int64) for lo, hi in gap_ranges]
    return np.unique(np.concatenate(pts + [np.zeros(1, dtype=np.int64)]))


def replay_run(run, c, cols, elections, edges, a0):
    """The model fed with chain ``c`` of a FlipRun: its event log, ``stats()`` and the window-start
    assignment ``a0`` [n] (the initial state, or ``run.state()[c]`` read at the last reset)."""
    st = run.stats()
    ev = run.events(c)
    return replay(a0, ev["t"], ev["v"], ev["target"], int(st["series_t0"][c]), int(st["steps"][c]), cols,
                  elections, edges, run.cfg.k)


KEYS = ("tally_now", "tally_sum", "seats_hist", "wins_sum", "gap_sum")


def assert_matches(got, i, exp, with_hist=True):
    """Entry ``i`` of a ``FlipRun.election_series`` result equals the model's ``exp``, bit for bit,
    and every histogram row sums to the window's yields."""
    assert int(got["yields"][i]) == exp["yields"]
    for key in KEYS:
        assert np.array_equal(got[key][i], exp[key]), (key, got[key][i], exp[key])
    assert (got["seats_hist"][i].sum(axis=-1) == exp["yields"]).all()
    if with_hist:
        assert np.array_equal(got["gap_hist"][i], exp["gap_hist"]), ("gap_hist", got["gap_hist"][i], exp["gap_hist"])
        assert (got["gap_hist"][i].sum(axis=-1) == exp["yields"]).all()
