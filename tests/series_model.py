"""Plain Python / numpy reference of the series read-outs of ``csrc/fc_series.hip``: the frame
slope / angle series per event, its change points, and the per-yield |cut| list whose lag sums and
autocorrelation ``oracle.flipref.acf_exact`` forms.  It shares no code with the kernels and does
not follow their schedule: every entry is computed from the state it belongs to.

:func:`queue_profile` alone restates a schedule, the documented one of the change-point modes
(four waves, 64-event chunks, a candidate queue flushed 64 at a time).  It is coverage bookkeeping
for ``series_cases``: it says which queue paths a case's oracle run would take a kernel through.
No expected value depends on it.
"""
import math

import numpy as np

WAVES = 4    # waves per chain of the frame-series kernel
CHUNK = 64   # events per chunk (one per lane)
NO_KEY = -1  # fewer than two cut frame edges


def frame_dense(a0, events, fu, fv, mid, centre):
    """The frame series of one chain's window: one entry for the window start (state ``a0``) and
    one after each event (``events[:, 1]`` the node, ``events[:, 4]`` its new district).

    Per entry: ``n_cut``, the cut frame edges (``a[fu[j]] != a[fv[j]]``); ``key``, the first two of
    them in frame order as ``j0 | j1 << 16`` (``NO_KEY`` with fewer than two); ``slope``,
    ``(by - ay) / (bx - ax)`` of their midpoints a, b in float64, ``+inf`` when ``bx == ax``;
    ``angle``, ``atan2(|cross|, dot)`` of the two midpoints relative to ``centre`` (well conditioned
    everywhere, unlike ``arccos`` of the normalised dot product), NaN when either midpoint is the
    centre.  Slope and angle are NaN with fewer than two cut frame edges."""
    a = np.array(a0, dtype=np.int64)
    fu = np.asarray(fu, dtype=np.int64)
    fv = np.asarray(fv, dtype=np.int64)
    mid = np.asarray(mid, dtype=np.float64).reshape(-1, 2)
    cx, cy = float(centre[0]), float(centre[1])
    E = len(events)
    n_cut = np.zeros(E + 1, dtype=np.int64)
    key = np.full(E + 1, NO_KEY, dtype=np.int64)
    slope = np.full(E + 1, np.nan)
    angle = np.full(E + 1, np.nan)
    values = {}  # (j0, j1) -> (slope, angle)
    for i in range(E + 1):
        if i:
            a[int(events[i - 1][1])] = int(events[i - 1][4])
        cut = np.nonzero(a[fu] != a[fv])[0]
        n_cut[i] = cut.size
        if cut.size < 2:
            continue
        j0, j1 = int(cut[0]), int(cut[1])
        key[i] = j0 | (j1 << 16)
        if (j0, j1) not in values:
            ax, ay, bx, by = float(mid[j0, 0]), float(mid[j0, 1]), float(mid[j1, 0]), float(mid[j1, 1])
            s = (by - ay) / (bx - ax) if bx != ax else math.inf
            pax, pay, pbx, pby = ax - cx, ay - cy, bx - cx, by - cy
            if (pax == 0.0 and pay == 0.0) or (pbx == 0.0 and pby == 0.0):
                an = math.nan
            else:
                an = math.atan2(abs(pax * pby - pay * pbx), pax * pbx + pay * pby)
            values[(j0, j1)] = (s, an)
        slope[i], angle[i] = values[(j0, j1)]
    return {"n_cut": n_cut, "key": key, "slope": slope, "angle": angle}


def _bits(x):
    """Bit patterns of float64 values, every NaN the same one."""
    x = np.array(x, dtype=np.float64)
    x[np.isnan(x)] = np.nan
    return x.view(np.int64)


def frame_changes(dense, t0, event_t):
    """The change points of a dense series: the window start (yield ``t0``) and every entry whose
    (slope, angle) differs from the previous entry's, with the yield of its event.  Values differ
    when their bit patterns do (-0.0 is not 0.0), except that NaN equals NaN.  Returns ``index``
    (entries of the dense series), ``t``, ``slope``, ``angle``."""
    s, a = _bits(dense["slope"]), _bits(dense["angle"])
    keep = np.ones(s.size, dtype=bool)
    keep[1:] = (s[1:] != s[:-1]) | (a[1:] != a[:-1])
    t_all = np.concatenate([[int(t0)], np.asarray(event_t, dtype=np.int64)])
    assert t_all.size == s.size
    idx = np.nonzero(keep)[0]
    return {"index": idx, "t": t_all[idx], "slope": np.asarray(dense["slope"])[idx],
            "angle": np.asarray(dense["angle"])[idx]}


def queue_profile(keys):
    """The candidate queues of the change-point modes over one chain's window, by the documented
    schedule.  ``keys[0]`` is the window start's key and ``keys[1:]`` the events'.  The ``ne``
    events form ``nk = ceil(ne / 64)`` chunks; wave ``w`` of four owns chunks
    ``[nk w / 4, nk (w + 1) / 4)``.  A candidate is an event whose key differs from the previous
    event's (the window start's for the first).  A wave queues its candidates chunk by chunk,
    flushes 64 of them whenever it holds 64 or more, and flushes what is left at its range's end.
    Returns ``(rests, tails)``: the queue length left after every 64-flush, in schedule order, and
    the four lengths at the ranges' ends (0: a wave that ends with an empty queue)."""
    keys = np.asarray(keys, dtype=np.int64)
    ne = keys.size - 1
    cand = keys[1:] != keys[:-1]
    nk = (ne + CHUNK - 1) // CHUNK
    rests, tails = [], []
    for w in range(WAVES):
        qn = 0
        for k in range(nk * w // WAVES, nk * (w + 1) // WAVES):
            qn += int(cand[CHUNK * k:CHUNK * (k + 1)].sum())
            if qn >= CHUNK:
                qn -= CHUNK
                rests.append(qn)
        tails.append(qn)
    return rests, tails


def cut_yields(x0, events, t0, T):
    """|cut| at the ``T`` yields ``t0 .. t0 + T - 1`` of a window: ``x0`` until the first event,
    then each event's ``cut`` (``events[:, 2]``) from its yield ``events[:, 0]`` on."""
    x = np.full(int(T), int(x0), dtype=np.int64)
    for ev in events:
        at = int(ev[0]) - int(t0)
        assert 0 < at < T
        x[at:] = int(ev[2])
    return x
