"""Host model of the short-bursts selection (include/flipchain.h
``fc_run_burst_select``), computed from the **list of per-yield states** by the definition, in the
style of recom_log_model.py: tallies by ``cols[a == d].sum()``, Python integers, the last index of
the best value.  No event, no replay.

For a ReCom case the states come from ``recom_log_model.states`` (one oracle run per yield); for a
flip run, ``states_from_events`` applies the run's ``fc_run_read_events`` log one event at a time
to the window-start plan and keeps the state at every yield.
"""
import dataclasses

import numpy as np

COUNT, GAP, CUT = "count", "gap", "cut"


@dataclasses.dataclass(frozen=True)
class Metric:
    kind: str
    col_a: int = 0
    col_b: int = 1
    num: int = 1
    den: int = 2
    maximize: bool = True


def tallies(a, cols, col, k):
    """District tallies of column ``col`` as Python integers."""
    cols = np.asarray(cols)
    return [int(cols[np.asarray(a) == d, col].sum()) for d in range(k)]


def score_of(metric, ta, tb, cut):
    """The score of one state from its tallies and |cut|, in Python integers."""
    if metric.kind == COUNT:
        return sum(1 for x, y in zip(ta, tb) if metric.den * x > metric.num * (x + y))
    if metric.kind == GAP:
        g = 0
        for x, y in zip(ta, tb):
            if x > y:
                g += 3 * y - x
            elif x < y:
                g += y - 3 * x
        return abs(g)
    return abs(int(cut))


def scores(metric, S, cut, cols, k):
    """The score of every state of S (``cut``: |cut| per state)."""
    if metric.kind == CUT:
        return [score_of(metric, None, None, c) for c in cut]
    return [score_of(metric, tallies(a, cols, metric.col_a, k), tallies(a, cols, metric.col_b, k), 0) for a in S]


def select_scored(sc, maximize, S, t0, cut, nb):
    """The selection over a window whose yields t0 .. have the scores ``sc``: the best value and the
    LAST index that has it."""
    best = max(sc) if maximize else min(sc)
    i = max(j for j, x in enumerate(sc) if x == best)
    return {"best_score": best, "best_t": t0 + i, "start_score": sc[0], "end_score": sc[-1], "best_cut": int(cut[i]),
            "best_nb": int(nb[i]), "best_plan": np.asarray(S[i], dtype=np.int8), "scores": sc, "ties": sc.count(best)}


def select(metric, S, t0, cut, nb, cols, k):
    """fc_run_burst_select of one chain whose window's yields t0 .. t0 + len(S) - 1 have the states
    S (``cut`` / ``nb``: per state)."""
    return select_scored(scores(metric, S, cut, cols, k), metric.maximize, S, t0, cut, nb)


def states_from_events(a0, ev, t0, steps, cut0, nb0):
    """Per-yield states, |cut| and |B| of a window t0 .. steps whose log is ``ev`` (``FlipRun.events``),
    one event applied at a time: the state at yield t has every event of t_e <= t."""
    a = np.asarray(a0, dtype=np.int64).copy()
    S, cut, nb = [], [], []
    j, c, b = 0, int(cut0), int(nb0)
    for t in range(int(t0), int(steps) + 1):
        while j < len(ev) and int(ev["t"][j]) <= t:
            a[int(ev["v"][j])] = int(ev["target"][j])
            c, b = int(ev["cut"][j]), int(ev["nb"][j])
            j += 1
        S.append(a.copy())
        cut.append(c)
        nb.append(b)
    assert j == len(ev)
    return S, cut, nb


def assert_matches(got, i, exp):
    """Row i of ``FlipRun.burst_select``'s result against ``select``'s."""
    for key in ("best_score", "best_t", "start_score", "end_score", "best_cut", "best_nb"):
        assert int(got[key][i]) == int(exp[key]), (key, i, int(got[key][i]), int(exp[key]))
    if "best_plan" in got:
        assert np.array_equal(got["best_plan"][i], exp["best_plan"]), ("best_plan", i)
