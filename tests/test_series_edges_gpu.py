"""GPU parity of the series kernels (``csrc/fc_series.hip``) with a plain reference at small shapes
and on every branch.

Every case of ``series_cases.CASES`` (what each is for, and that the oracle's run reaches it:
test_series_cases.py) runs on the device, and at every read of the case every chain is compared:

1. the event log with the C oracle's events (t, v, cut, nb, target), exactly;
2. ``frame_series`` with ``series_model.frame_dense``: length and ``n_cut`` exact, NaN where the
   model has NaN, the slope with ``==`` (both divide the same two float64 differences once), the
   angle within ``ANGLE_TOL`` (the device takes ``acos`` of a cosine a few ulp off, which near +-1
   is an angle error of sqrt(2 * 1e-15), about 5e-8; the model's ``atan2`` form is accurate to
   about 1e-15);
3. ``frame_series_changes`` in both forms -- the staged single pass of a default run and the count
   / write passes of an identically built run with ``FC_FLAG_SERIES_TWO_PASS`` -- with
   ``series_model.frame_changes``: offsets and yields exact, values by rule 2, and bitwise the
   device's own dense series at those entries; a chain sub-range gives the whole run's rows;
4. ``autocorr`` with ``oracle.flipref.acf_exact`` on the model's per-yield |cut| list: lag sums and
   ACF bit for bit, and ``autocorr_pairs`` = max(0, T - L).

Once, not per case: the run's cache of the frame tables (a sequence of frames on one run against
fresh runs) and the calls the entry points refuse.

Not covered here: the multi-batch path of ``fc_run_autocorr`` (more than 2^29 yields in a batch),
chains of unequal window length in one call (all chains of a run take the same steps), and ReCom
bursts in the expansion kernel (test_recom_log_gpu.py).
"""
import dataclasses

import numpy as np
import pytest

import series_cases as SC
import series_model as M
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.engine import EVENT_DTYPE, FlipGraph, FlipRun, RunConfig
from oracle.flipref import acf_exact
from test_slope_gpu import ANGLE_TOL

pytestmark = pytest.mark.gpu

EVENT_FIELDS = ("t", "v", "cut", "nb", "target")
assert all(f in EVENT_DTYPE.names for f in EVENT_FIELDS)


def _run(case, flags=0):
    """The case's run, taken to the opening of its window."""
    fg = FlipGraph(case.spec)
    lo, hi = case.bounds()
    nc = case.n_chains
    cfg = RunConfig(seed=case.seed, pop_lo=lo, pop_hi=hi, diag_mask=_lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES,
                    event_cap=case.steps + 8, flags=flags)
    run = FlipRun(fg, np.stack([case.plan(c) for c in range(nc)]), cfg, bases=[case.base(c) for c in range(nc)])
    if case.pre is not None:
        if case.pre:
            run.steps(case.pre)
        run.series_reset()
    return fg, run


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _values_match(who, got_s, got_a, want_s, want_a):
    """Rule 2 on slope / angle arrays; returns the largest angle deviation."""
    assert got_s.shape == want_s.shape and got_a.shape == want_a.shape, who
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s)), who
    assert np.array_equal(np.isnan(got_a), np.isnan(want_a)), who
    ok = ~np.isnan(want_s)
    bad = np.nonzero(got_s[ok] != want_s[ok])[0]
    assert bad.size == 0, (who, "slope", bad[:3], got_s[ok][bad[:3]], want_s[ok][bad[:3]])
    ok = ~np.isnan(want_a)
    dev = np.abs(got_a[ok] - want_a[ok])
    worst = float(dev.max()) if dev.size else 0.0
    assert worst <= ANGLE_TOL, (who, "angle", int(dev.argmax()), worst)
    return worst


def _check_read(case, run, s, staged):
    """Everything the case reads after s window steps; returns the largest angle deviation."""
    C = case.n_chains
    win = [case.window(c, s) for c in range(C)]
    worst = 0.0
    for c in range(C):
        ev, want = run.events(c), win[c]["events"]
        assert len(ev) == len(want), (case.name, s, c, len(ev), len(want))
        for j, f in enumerate(EVENT_FIELDS):
            assert np.array_equal(ev[f].astype(np.int64), want[:, j]), (case.name, s, c, f)
    st = run.stats()
    assert np.all(st["series_t0"] == case.t0) and np.all(st["steps"] == case.t0 + s)
    for fname, frame in case.frame_set().items():
        model = [case.dense(c, fname, s) for c in range(C)]
        dense = run.frame_series(frame)
        for c in range(C):
            who = (case.name, s, fname, c)
            n = len(win[c]["events"]) + 1
            assert int(dense["len"][c]) == n == len(model[c]["n_cut"]), who
            assert np.array_equal(dense["n_cut"][c, :n], model[c]["n_cut"]), who
            worst = max(worst, _values_match(who, dense["slope"][c, :n], dense["angle"][c, :n], model[c]["slope"],
                                             model[c]["angle"]))
        whole = run.frame_series_changes(frame)
        assert run.diag_paths()["series_staged"] == (1 if staged else 0)
        assert whole["offsets"][0] == 0 and len(whole["offsets"]) == C + 1
        for c in range(C):
            who = (case.name, s, fname, c, "changes")
            want = M.frame_changes(model[c], case.t0, win[c]["events"][:, 0])
            lo, hi = int(whole["offsets"][c]), int(whole["offsets"][c + 1])
            assert hi - lo == len(want["t"]), who
            assert np.array_equal(whole["t"][lo:hi], want["t"]), who
            worst = max(worst, _values_match(who, whole["slope"][lo:hi], whole["angle"][lo:hi], want["slope"],
                                             want["angle"]))
            for key in ("slope", "angle"):
                assert np.array_equal(_bits(whole[key][lo:hi]), _bits(dense[key][c][want["index"]])), who + (key,)
        part = run.frame_series_changes(frame, c0=1, nc=C - 2)
        lo, hi = int(whole["offsets"][1]), int(whole["offsets"][C - 1])
        assert np.array_equal(part["offsets"], whole["offsets"][1:C] - lo), (case.name, s, fname)
        assert np.array_equal(part["t"], whole["t"][lo:hi])
        for key in ("slope", "angle"):
            assert np.array_equal(_bits(part[key]), _bits(whole[key][lo:hi])), (case.name, s, fname, key)
        query = run.frame_series_changes(frame, query=True)
        assert np.array_equal(query["offsets"], whole["offsets"])
    T = s + 1
    lags = SC.lags_for(T)
    sums, acf = run.autocorr(lags)
    pairs = run.autocorr_pairs(lags)
    for c in range(C):
        x = case.info(c)["x"][:T]
        want_sums, want_acf = acf_exact(x, lags)
        assert np.array_equal(sums[c], want_sums), (case.name, s, c, lags, sums[c], want_sums)
        assert np.array_equal(_bits(acf[c]), _bits(want_acf)), (case.name, s, c, lags, acf[c], want_acf)
        assert pairs[c].tolist() == [max(0, T - L) for L in lags]
    return worst


# (a case that reads no frame makes no change-point call: one form)
PARAMS = [(c.name, form) for c in SC.CASES for form in ("staged", "two passes")
          if form == "staged" or c.frames is not SC.no_frames]


@pytest.mark.parametrize("name,form", PARAMS)
def test_series_case_matches_reference(gpu, name, form):
    case = SC.BY_NAME[name]
    staged = form == "staged"
    fg, run = _run(case, flags=0 if staged else _lib.FC_FLAG_SERIES_TWO_PASS)
    worst = 0.0
    for parts, s in case.launches():
        for p in parts:
            run.steps(p)
        worst = max(worst, _check_read(case, run, s, staged))
    for c in range(case.n_chains):
        assert np.array_equal(run.state()[c], case.oracle(c)["final"]), (name, c)
    if case.frame_set():
        print(f"{name} ({form}): largest angle deviation {worst:.3e}")
    run.close()
    fg.close()


def _read(run, frame):
    d = run.frame_series(frame)
    ch = run.frame_series_changes(frame)
    live = np.arange(d["slope"].shape[1])[None, :] < d["len"][:, None]
    return [d["len"], d["n_cut"][live], _bits(d["slope"][live]), _bits(d["angle"][live]), ch["offsets"], ch["t"],
            _bits(ch["slope"]), _bits(ch["angle"])]


def test_frame_tables_follow_the_frame(gpu):
    """The run keeps the frame tables of the last call and uploads them when the frame differs.
    One run reads frame A, frame B, A again, A's edges about another centre, A's edges with other
    midpoints and the empty frame; each read (both entry points) is bitwise the same read on a
    fresh run that has seen no other frame."""
    case = dataclasses.replace(SC.BY_NAME["cycle65 ladder"], pre=None, reads=(300,))
    frames = SC.cycle65_frames(case)
    A, B = frames["full"], frames["even"]
    reads = [A, B, A, dataclasses.replace(A, center=(0.3, -0.2)),
             dataclasses.replace(A, mid=A.mid * np.asarray([1.5, 0.75]) + 0.125), SC.ring_frame(case.spec, [])]
    fg, run = _run(case)
    run.steps(300)
    got = [_read(run, f) for f in reads]
    run.close()
    for j, f in enumerate(reads):
        fresh_fg, fresh = _run(case)
        fresh.steps(300)
        want = _read(fresh, f)
        for x, y in zip(got[j], want):
            assert np.array_equal(x, y), j
        fresh.close()
        fresh_fg.close()
    fg.close()
    # the reads differ from one another where the frames do: a stale table would have shown
    assert not np.array_equal(got[0][2], got[4][2]) and not np.array_equal(got[0][3], got[3][3])
    assert np.array_equal(got[0][2], got[3][2])  # the slope does not depend on the centre
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[2]))
    assert got[5][1].max() == 0 and np.all(got[5][4] == np.arange(case.n_chains + 1))


def test_series_calls_refused(gpu):
    case = dataclasses.replace(SC.BY_NAME["cycle256 word pairs"], reads=(10,))
    fg, run = _run(case)
    run.steps(10)
    ok = SC.ring_frame(case.spec, range(256))
    with pytest.raises(NotImplementedError):
        run.frame_series(SC.ring_frame(case.spec, list(range(256)) + [0]))
    with pytest.raises(NotImplementedError):
        run.frame_series_changes(SC.ring_frame(case.spec, list(range(256)) + [0]))
    loop = dataclasses.replace(ok, ev=ok.eu.copy())
    far = dataclasses.replace(ok, ev=np.where(np.arange(256) == 200, 256, ok.ev).astype(np.int32))
    low = dataclasses.replace(ok, eu=np.where(np.arange(256) == 3, -1, ok.eu).astype(np.int32))
    for bad in (loop, far, low):
        with pytest.raises(ValueError):
            run.frame_series(bad)
        with pytest.raises(ValueError):
            run.frame_series_changes(bad)
    with pytest.raises(ValueError):
        run.autocorr([1, -1])
    assert run.frame_series(ok)["len"].tolist() == [11] * case.n_chains  # the run is still good
    run.close()
    fg.close()
