"""Host model of the plan samples (include/flipchain.h): a plain numpy replay of one
chain's accepted-flip log up to a list of yields, by the definitions.  It shares no code with the
device path; tests/test_plans.py checks it against a per-yield recomputation of an oracle chain,
tests/test_plans_gpu.py checks the device against it.

One Python loop over the samples; the events up to a sample's yield are applied by index (numpy
keeps the last of several assignments to one index, which is the log order)."""
import numpy as np

CHUNK = 64  # the device reads its log in chunks of this many events


def events_array(ev):
    """``FlipRun.events()`` (a structured array) as the oracle's [m, 5] int64 rows
    (t, v, cut, nb, target)."""
    return np.stack([ev["t"], ev["v"], ev["cut"], ev["nb"], ev["target"]], axis=1).astype(np.int64).reshape(-1, 5)


def replay(a0, events, t0, T, series_cut0, series_nb0, pop, times, k=None):
    """``a0`` [n] district indices at yield ``t0``; ``events`` [m, 5] rows (t, v, cut, nb, target)
    in log order, event i making ``a[v] = target`` from yield ``t`` on; window yields ``t0 .. T``;
    ``pop`` [n]; ``times`` strictly increasing yields inside the window.  Returns the outputs of
    ``fc_run_sample_plans`` for this chain -- ``plans`` int8 [m, n], ``cut``, ``nb``, ``dist0`` int64
    [m], ``pops`` int64 [m, k] -- and two counts of what the log asks of the device:
    ``chunk_same_node`` (events whose node already occurred in their chunk of 64, chunks counted
    from the window's first event) and ``repeat_between`` (intervals between consecutive samples,
    the first from the window start, that hold two events on one node)."""
    a0 = np.asarray(a0, dtype=np.int64)
    events = np.asarray(events, dtype=np.int64).reshape(-1, 5)
    pop = np.asarray(pop, dtype=np.int64)
    times = np.asarray(times, dtype=np.int64)
    k = int(max(a0.max(), events[:, 4].max() if len(events) else 0)) + 1 if k is None else int(k)
    et, evv, etg = events[:, 0], events[:, 1], events[:, 4]
    if len(events):
        assert et[0] > t0 and et[-1] <= T and (np.diff(et) > 0).all()
    if times.size:
        assert times[0] >= t0 and times[-1] <= T and (np.diff(times) > 0).all()
    m = times.size
    plans = np.zeros((m, a0.size), dtype=np.int8)
    cut, nb, dist0 = (np.zeros(m, dtype=np.int64) for _ in range(3))
    pops = np.zeros((m, k), dtype=np.int64)
    a = a0.copy()
    lo = 0
    repeat_between = 0
    for j in range(m):
        hi = int(np.searchsorted(et, times[j], side="right"))  # events with t_e <= times[j]
        a[evv[lo:hi]] = etg[lo:hi]
        repeat_between += int(np.unique(evv[lo:hi]).size < hi - lo)
        lo = hi
        plans[j] = a
        cut[j] = events[hi - 1, 2] if hi else series_cut0
        nb[j] = events[hi - 1, 3] if hi else series_nb0
        dist0[j] = int((a != a0).sum())
        pops[j] = np.bincount(a, weights=pop, minlength=k).astype(np.int64)
    same = 0
    for c in range(0, len(events), CHUNK):
        chunk = evv[c:c + CHUNK]
        same += int(chunk.size - np.unique(chunk).size)
    return {"plans": plans, "cut": cut, "nb": nb, "dist0": dist0, "pops": pops,
            "chunk_same_node": same, "repeat_between": repeat_between}


def replay_run(run, c, a0, times):
    """The model fed with chain ``c`` of a FlipRun: its event log, ``stats()`` and the window-start
    assignment ``a0`` [n] (the initial state, or ``run.state()[c]`` read at the last reset)."""
    st = run.stats()
    return replay(a0, events_array(run.events(c)), int(st["series_t0"][c]), int(st["steps"][c]),
                  int(st["series_cut0"][c]), int(st["series_nb0"][c]), run.graph.spec.pop, times, run.cfg.k)


KEYS = ("plans", "cut", "nb", "dist0", "pops")


def assert_matches(got, i, exp):
    """Entry ``i`` of a ``FlipRun.sample_plans`` result equals the model's ``exp``, bit for bit."""
    for key in KEYS:
        if key not in got:
            continue
        assert got[key][i].shape == exp[key].shape and got[key][i].dtype == exp[key].dtype, (key, got[key][i].shape)
        assert np.array_equal(got[key][i], exp[key]), (key, np.argwhere(got[key][i] != exp[key])[:5])
