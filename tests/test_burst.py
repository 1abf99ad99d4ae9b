"""CPU checks of the short-bursts metric rule: ``fc_burst_eval`` -- the rule the
replay kernel applies, compiled for the host -- against Python integers, the metric checks, the
LDS-fit predicate at its edge, and the coverage of the case table that tests/test_burst_gpu.py
compares on the device (a failed condition there means the case is wrong: change the case, never
the condition).  No GPU."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import burst_model as BM
import recom_cases as RC
import recom_log_model as M
from flipcomplexityempirical_amd import build as B
from flipcomplexityempirical_amd.engine import BurstMetric

COLS_SEED = 11
CASES = ("reject 8x8 k=4", "size 8x8 k=4")


def _dev(m):
    return BurstMetric(kind=m.kind, col_a=m.col_a, col_b=m.col_b, num=m.num, den=m.den, maximize=m.maximize)


def _both(m, a, b, cut=0):
    got = _dev(m).eval(a, b, cut)
    assert got == BM.score_of(m, [int(x) for x in a], [int(x) for x in b], cut)
    return got


# ---- fc_burst_eval ----------------------------------------------------------------------------
def test_count_half_is_seats_and_a_tie_is_no_win():
    m = BM.Metric(BM.COUNT)
    assert _both(m, [5, 4, 7, 0], [4, 5, 7, 0]) == 1  # a win, a loss, a tie, an empty district
    assert _both(m, [1, 1, 1], [0, 0, 0]) == 3
    assert _both(m, [3], [3]) == 0


def test_count_threshold_met_with_equality_is_not_counted():
    m = BM.Metric(BM.COUNT, num=2, den=5)
    assert _both(m, [2], [3]) == 0          # 5 * 2 == 2 * 5
    assert _both(m, [21], [29]) == 1        # 105 > 100
    assert _both(m, [40, 39, 41], [60, 61, 59]) == 1
    m = BM.Metric(BM.COUNT, num=3, den=4)
    assert _both(m, [3, 30, 31], [1, 10, 10]) == 1
    big = BM.Metric(BM.COUNT, num=2 ** 20 - 1, den=2 ** 20)
    assert _both(big, [2 ** 20 - 1, 2 ** 20], [1, 0]) == 1


def test_gap_is_the_election_rule_and_absolute():
    m = BM.Metric(BM.GAP, maximize=False)
    assert _both(m, [5, 4, 7], [4, 5, 7]) == abs((3 * 4 - 5) + (5 - 3 * 4))
    assert _both(m, [10, 10], [1, 2]) == abs((3 - 10) + (6 - 10))  # a negative sum
    assert _both(m, [1, 2], [10, 10]) == (10 - 3 * 1) + (10 - 3 * 2)
    rng = np.random.default_rng(3)
    for _ in range(50):
        k = int(rng.integers(1, 33))
        a, b = rng.integers(0, 2 ** 31, k), rng.integers(0, 2 ** 31, k)
        _both(m, a, b)
        _both(BM.Metric(BM.COUNT, num=int(rng.integers(1, 7)), den=7), a, b)


def test_cut_needs_no_columns():
    m = BM.Metric(BM.CUT, maximize=False)
    assert _dev(m).eval(cut=17) == 17 == BM.score_of(m, None, None, 17)
    assert _dev(m).eval([1, 2], [3, 4], cut=0) == 0


def test_overflow_bound():
    """den * total = 2^62 is refused, one below it accepted; the products are then exact."""
    m = BM.Metric(BM.COUNT, num=2 ** 20 - 1, den=2 ** 20)
    top = 2 ** 42
    with pytest.raises(ValueError, match="2\\^62"):
        _dev(m).eval([top - 5, 3], [1, 1])
    assert _both(m, [top - 5, 3], [0, 1]) == 1
    assert _both(BM.Metric(BM.GAP), [top - 5, 3], [0, 1]) == abs(-(top - 5) + 3 - 3)
    with pytest.raises(ValueError, match="2\\^62"):
        _dev(BM.Metric(BM.GAP, den=4)).eval([2 ** 60], [0])
    assert _both(BM.Metric(BM.GAP, den=4), [2 ** 60 - 1], [0]) == 2 ** 60 - 1
    with pytest.raises(ValueError, match="2\\^62"):
        _dev(BM.Metric(BM.GAP)).eval([2 ** 62], [0])


def test_bad_metrics():
    for bad, what in ((BurstMetric(kind=7), "unknown kind"), (BurstMetric(kind="count", num=2, den=2), "num < den"),
                      (BurstMetric(kind="count", num=0, den=2), "num < den"),
                      (BurstMetric(kind="gap", num=1, den=2 ** 20 + 1), "2\\^20"),
                      (BurstMetric(kind="cut", maximize=2), "maximize")):
        with pytest.raises(ValueError, match=what):
            bad.eval([1], [1])
    with pytest.raises(ValueError, match="unknown metric kind"):
        BurstMetric(kind="seats").struct()
    with pytest.raises(ValueError, match="negative"):
        BurstMetric(kind="count").eval([-1], [1])
    with pytest.raises(ValueError, match="k must be"):
        BurstMetric(kind="count").eval(np.zeros(33), np.zeros(33))


# ---- the HIP-free header: metric checks against a run's columns, and the LDS fit ---------------
def test_header_checks_without_hip():
    """fc_burst.h compiles as plain C++ (g++, no HIP header) and its checks hold at their edges."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "burst_check.cpp")
    with tempfile.TemporaryDirectory(prefix="fc_burst_") as tmp:
        exe = os.path.join(tmp, "burst_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", B.CSRC, "-o", exe, src],
                       check=True, timeout=120)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got = dict(line.split("=", 1) for line in out.strip().splitlines())
    assert got["good"] == got["col_b_last"] == got["cut_ignores_columns"] == got["below_bound"] == "ok"
    for key in ("col_b_is_n_cols", "same_columns", "negative_column"):
        assert "columns below n_cols" in got[key], key
    assert got["unknown_kind"] == "unknown kind" and "2^62" in got["at_bound"]
    assert got["fit"] == "101 bytes=49152"  # 48 KB exactly fits, 16 bytes more do not


# ---- coverage of the case table ----------------------------------------------------------------
def cols_of(case):
    return np.random.default_rng(COLS_SEED).integers(0, 50, (case.spec.n, 2))


METRICS = {"count": BM.Metric(BM.COUNT), "gap": BM.Metric(BM.GAP, maximize=False), "cut": BM.Metric(BM.CUT, maximize=False)}


@functools.lru_cache(maxsize=None)
def table(name):
    """Per chain of the case: the model's selection under each of the three metrics, and the burst
    lengths of its expected log.  Computed once, shared, not changed."""
    case = RC.BY_NAME[name]
    cols, out = cols_of(case), []
    for c in range(case.n_chains):
        S, full = M.states(case, c)
        cut, nb = M.cut_nb(case.spec, S)
        _, lens = M.expected_log(S, 0, cut, nb)
        sel = {key: BM.select(m, S, 0, cut, nb, cols, case.k) for key, m in METRICS.items()}
        out.append(dict(S=S, sel=sel, lens=lens, flags=M.valid_flags(full)))
    return out


def _held(ch, key):
    """Whether best_t is a yield a rejected step made: the best state was reached before it."""
    t = ch["sel"][key]["best_t"]
    return t > 0 and ch["flags"][t - 1] == 1 and np.array_equal(ch["S"][t], ch["S"][t - 1])


def test_case_table_coverage():
    rej, siz = table(CASES[0]), table(CASES[1])
    T = RC.BY_NAME[CASES[0]].steps
    assert len(rej) == len(siz) == 5 and T == 40
    best_t = {(name, key): [ch["sel"][key]["best_t"] for ch in tab] for name, tab in ((0, rej), (1, siz))
              for key in METRICS}
    every = [t for ts in best_t.values() for t in ts]
    # a best at the window start, a best at its end, interior bests
    assert 0 in best_t[0, "gap"] and T in best_t[0, "count"] and T in best_t[0, "cut"]
    assert any(0 < t < T for t in best_t[0, "gap"]) and any(0 < t < T for t in best_t[0, "cut"])
    assert all(0 < t < T for t in best_t[1, "gap"])
    assert 0 in every and T in every
    # COUNT rises above its start score and many yields tie at the best
    for ch in rej:
        s = ch["sel"]["count"]
        assert s["best_score"] > s["start_score"] and s["ties"] >= 2
    assert any(ch["sel"][key]["ties"] >= 2 and 0 < ch["sel"][key]["best_t"] < T for ch in rej + siz for key in METRICS)
    # rejected steps after the best: best_t is a re-yield of the best state, inside the window and at its end
    assert any(_held(ch, key) and ch["sel"][key]["best_t"] < T for ch in rej for key in METRICS)
    assert any(_held(ch, key) and ch["sel"][key]["best_t"] == T for ch in rej for key in METRICS)
    # bursts across a 64-event chunk boundary, in every chain
    assert all(M.straddles(ch["lens"]) >= 1 for ch in rej + siz)
