"""GPU checks of the short-bursts selection and rewind: ``FlipRun.burst_select``
against tests/burst_model.py, which scores the **per-yield states** by the definition and takes
the last index of the best value (no event, no replay).  The ReCom states come from one oracle
run per yield (recom_log_model.states); a flip run's from its ``events()`` applied one at a time.
tests/test_burst.py checks on the CPU that the case table holds a best at the window start, at
its end and inside it, ties, rejected steps after the best and bursts across a chunk boundary.
Everything is compared bit for bit, for every chain."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest

import burst_model as BM
import recom_cases as RC
import recom_log_model as M
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd import optimization as O
from flipcomplexityempirical_amd.engine import EVENT_DTYPE, STAT_FIELDS, BurstMetric, FlipGraph, FlipRun, RunConfig
from test_burst import METRICS, cols_of, table

pytestmark = pytest.mark.gpu

SERIES = _lib.FC_DIAG_SERIES
CASES = ("reject 8x8 k=4", "size 8x8 k=4", "size 13x5 k=4", "weights 9x7 k=3", "k=32 16x16", "cycle C32")
# COUNT at 1/2 and 2/5, GAP and CUT, each in both senses
ALL_METRICS = [BM.Metric(kind, num=num, den=den, maximize=mx)
               for kind, num, den in ((BM.COUNT, 1, 2), (BM.COUNT, 2, 5), (BM.GAP, 1, 2), (BM.CUT, 1, 2))
               for mx in (True, False)]
WINDOW = ("events", "series_t0", "series_cut0", "series_nb0")  # what a rewind restarts


def _dev(m):
    return BurstMetric(kind=m.kind, col_a=m.col_a, col_b=m.col_b, num=m.num, den=m.den, maximize=m.maximize)


def _run(case, event_cap, trace=False, seed=RC.SEED):
    nc = case.n_chains
    lohi = np.asarray([case.chain_bounds(c) for c in range(nc)], dtype=np.int64)
    cfg = RunConfig(k=case.k, labels=tuple(range(case.k)), proposal=_lib.FC_PROPOSE_RECOM, seed=seed,
                    pop_lo=int(lohi[0, 0]), pop_hi=int(lohi[0, 1]), base=case.base, chain_id_offset=case.chain_id_offset,
                    recom_pop_target=case.pop_target, recom_epsilon=case.epsilon, recom_node_repeats=case.node_repeats,
                    recom_max_attempts=case.max_attempts, diag_mask=SERIES, event_cap=event_cap,
                    trace_chains=nc if trace else 0, trace_cap=4096 if trace else 0)
    return FlipRun(FlipGraph(case.spec), np.stack([case.plan(c) for c in range(nc)]), cfg,
                   pop_bounds=lohi if len(case.bounds()) > 1 else None)


def _events(run, c):
    """The events of chain c the log holds (an overflowed log: its first event_cap events)."""
    cap = int(run.cfg.event_cap)
    out = np.zeros(cap, dtype=EVENT_DTYPE)
    n = ctypes.c_int64(0)
    rc = _lib.load().fc_run_read_events(run.handle, c, ctypes.cast(out.ctypes.data, ctypes.POINTER(_lib.Event)), cap,
                                        ctypes.byref(n))
    assert rc == 0
    return out[:min(cap, n.value)].tobytes()


def _snapshot(run):
    """Everything a select without rewind must leave as it was."""
    st = run.stats()
    return dict(blob=run.checkpoint(), state=run.state(), stats={f: st[f].copy() for f in STAT_FIELDS},
                events=[_events(run, c) for c in range(run.n_chains)])


def _assert_unchanged(run, snap, chains=None):
    st, state = run.stats(), run.state()
    sel = list(range(run.n_chains)) if chains is None else list(chains)
    for f in STAT_FIELDS:
        assert np.array_equal(st[f][sel], snap["stats"][f][sel]), f
    assert np.array_equal(state[sel], snap["state"][sel])
    for c in sel:
        assert _events(run, c) == snap["events"][c], c
    if chains is None:
        assert run.checkpoint() == snap["blob"]


@functools.lru_cache(maxsize=None)
def _states(name):
    """Per chain of the case: the per-yield states, |cut| and |B|.  Computed once, shared, not changed."""
    case = RC.BY_NAME[name]
    out = []
    for c in range(case.n_chains):
        S, _ = M.states(case, c)
        cut, nb = M.cut_nb(case.spec, S)
        out.append((S, cut, nb))
    return out


def _check_window(run, case, t0, metrics=ALL_METRICS):
    cols, steps = cols_of(case), run.stats()["steps"]
    for m in metrics:
        got = run.burst_select(_dev(m), plans=True)
        for c, (S, cut, nb) in enumerate(_states(case.name)):
            T = int(steps[c])
            BM.assert_matches(got, c, BM.select(m, S[t0:T + 1], t0, cut[t0:T + 1], nb[t0:T + 1], cols, case.k))


# ---- 1. select equals the model, nothing in the run changes -------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_select_equals_the_model(gpu, name):
    case = RC.BY_NAME[name]
    run = _run(case, case.steps * case.spec.n)
    run.set_elections(cols_of(case), [(0, 1)])
    # a window of 0 steps: the best is the start
    snap = _snapshot(run)
    got = run.burst_select(_dev(ALL_METRICS[0]), plans=True)
    assert (got["best_t"] == 0).all() and np.array_equal(got["best_score"], got["start_score"])
    assert np.array_equal(got["best_plan"], snap["state"]) and np.array_equal(got["end_score"], got["start_score"])
    _check_window(run, case, 0)
    _assert_unchanged(run, snap)
    run.steps(17).steps(case.steps - 17)
    snap = _snapshot(run)
    _check_window(run, case, 0)
    assert run.burst_select_ms() > 0
    # outputs are optional, and a sub-range reads its own chains
    got = run.burst_select(_dev(ALL_METRICS[4]), c0=1, nc=2)
    whole = run.burst_select(_dev(ALL_METRICS[4]))
    assert "best_plan" not in got and all(np.array_equal(got[key], whole[key][1:3]) for key in got)
    _assert_unchanged(run, snap)
    run.close()


def test_window_reopened_by_series_reset(gpu):
    """series_reset() after 15 steps, 25 more: the selection over yields 15 .. 40."""
    case = RC.BY_NAME["reject 8x8 k=4"]
    run = _run(case, case.steps * case.spec.n)
    run.set_elections(cols_of(case), [(0, 1)])
    run.steps(15)
    run.series_reset()
    run.steps(case.steps - 15)
    assert (run.stats()["series_t0"] == 15).all()
    snap = _snapshot(run)
    _check_window(run, case, 15)
    _assert_unchanged(run, snap)
    run.close()


# ---- 2. flip logs ----------------------------------------------------------------------------------
def _flip_run(spec, k, a0, bases, steps, pct, seed=17):
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, pct)
    cfg = RunConfig(k=k, labels=(-1, 1) if k == 2 else tuple(range(k)),
                    proposal=_lib.FC_PROPOSE_BI_SIGN if k == 2 else _lib.FC_PROPOSE_PAIR, seed=seed, pop_lo=lo, pop_hi=hi,
                    diag_mask=_lib.FC_DIAG_WAIT | SERIES, event_cap=steps + 1)
    return FlipRun(FlipGraph(spec), np.stack([a0] * len(bases)), cfg, bases=np.asarray(bases, dtype=np.float64))


@pytest.mark.parametrize("k", [2, 4])
def test_flip_logs(gpu, k):
    """A flip chain flips one node back and forth inside a chunk of 64 events (asserted from the
    events read); the rewind is refused and changes nothing."""
    if k == 2:
        spec = G.grid_graph(6, 6)
        a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 3), [-1, 1])
        run = _flip_run(spec, 2, a0, [1.0, 1.0, 1.0], 500, 0.5)
    else:
        spec = G.grid_graph(8, 8)
        a0 = spec.assignment_array(G.strip_plan(spec, 4), list(range(4)))
        run = _flip_run(spec, 4, a0, [1.0, 0.8, 1.0], 500, 0.5)
    cols = cols_of(RC.BY_NAME["size 8x8 k=4"])[:spec.n]
    run.set_elections(cols, [(0, 1)])
    start = run.state()
    run.steps(500)
    st = run.stats()
    snap = _snapshot(run)
    repeats = 0
    for c in range(run.n_chains):
        ev = run.events(c)
        assert len(ev) > 64
        repeats += sum(len(set(ev["v"][i:i + 64].tolist())) < len(ev["v"][i:i + 64]) for i in range(0, len(ev), 64))
        S, cut, nb = BM.states_from_events(start[c], ev, 0, int(st["steps"][c]), st["series_cut0"][c], st["series_nb0"][c])
        assert np.array_equal(S[-1], snap["state"][c])
        for m in ALL_METRICS:
            got = run.burst_select(_dev(m), c0=c, nc=1, plans=True)
            BM.assert_matches(got, 0, BM.select(m, S, 0, cut, nb, cols, k))
    assert repeats > 0
    with pytest.raises(NotImplementedError, match="ReCom chains only"):
        run.burst_select(_dev(ALL_METRICS[0]), rewind=True)
    _assert_unchanged(run, snap)
    run.close()


def test_flip_window_growing_event_by_event(gpu):
    """The walk takes a chunk event by event when more than 16 yields end in it and yield by yield
    otherwise.  A k = 2 window grown one step at a time has a last chunk of every length: the
    selection after every step, across both sides of that threshold (asserted from the events)."""
    spec = G.grid_graph(6, 6)
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 3), [-1, 1])
    run = _flip_run(spec, 2, a0, [1.0, 1.0], 500, 0.5)
    cols = cols_of(RC.BY_NAME["size 8x8 k=4"])[:spec.n]
    run.set_elections(cols, [(0, 1)])
    start = run.state()
    run.steps(300)
    metrics = [ALL_METRICS[0], ALL_METRICS[5], ALL_METRICS[7]]  # COUNT up, GAP down, CUT down
    got, lens = [], []
    for _ in range(100):
        run.steps(1)
        got.append([run.burst_select(_dev(m), plans=True) for m in metrics])
        lens.append(run.stats()["events"].copy())
    st = run.stats()
    tails = set()
    for c in range(run.n_chains):
        ev = run.events(c)
        assert len(set(ev["t"].tolist())) == len(ev)  # every event is a yield of its own
        S, cut, nb = BM.states_from_events(start[c], ev, 0, 400, st["series_cut0"][c], st["series_nb0"][c])
        tails |= {int(x[c]) % 64 for x in lens}
        for j, m in enumerate(metrics):
            sc = BM.scores(m, S, cut, cols, 2)
            for i in range(100):
                T = 301 + i
                exp = BM.select_scored(sc[:T + 1], m.maximize, S[:T + 1], 0, cut[:T + 1], nb[:T + 1])
                BM.assert_matches({key: val[c:c + 1] for key, val in got[i][j].items()}, 0, exp)
    assert {15, 16, 17, 18} <= tails
    run.close()


# ---- 3. a rewind writes exactly what it should -----------------------------------------------------
KEPT = ("draws", "steps", "proposals", "accepted", "inv_pop", "sum_cut", "sum_nb")


@pytest.mark.parametrize("key", ["count", "gap"])
def test_rewind_writes(gpu, key):
    case = RC.BY_NAME["reject 8x8 k=4"]
    m, tab = METRICS[key], table(case.name)
    run = _run(case, case.steps * case.spec.n)
    run.set_elections(cols_of(case), [(0, 1)])
    run.steps(case.steps)
    before = run.stats()
    got = run.burst_select(_dev(m), rewind=True, plans=True)
    st, state = run.stats(), run.state()
    for c, ch in enumerate(tab):
        exp = ch["sel"][key]
        BM.assert_matches(got, c, exp)
        assert np.array_equal(state[c], exp["best_plan"])
        cut, nb, _ = G.cut_and_boundary(case.spec, exp["best_plan"].astype(np.int64))
        assert (int(st["cut"][c]), int(st["nb"][c])) == (cut, nb)
        assert (int(st["series_cut0"][c]), int(st["series_nb0"][c])) == (cut, nb)
        assert int(st["events"][c]) == 0 and int(st["series_t0"][c]) == int(st["steps"][c]) == case.steps
        assert len(run.events(c)) == 0
    for f in KEPT:
        assert np.array_equal(st[f], before[f]), f
    # an immediate second select on the fresh window: the start is the best, at the same score
    again = run.burst_select(_dev(m), plans=True)
    assert (again["best_t"] == case.steps).all() and np.array_equal(again["best_score"], got["best_score"])
    assert np.array_equal(again["best_plan"], state) and np.array_equal(again["start_score"], got["best_score"])
    run.close()
    # a sub-range leaves the other chains bit-identical
    run = _run(case, case.steps * case.spec.n)
    run.set_elections(cols_of(case), [(0, 1)])
    run.steps(case.steps)
    snap = _snapshot(run)
    got = run.burst_select(_dev(m), rewind=True, c0=1, nc=2, plans=True)
    _assert_unchanged(run, snap, chains=(0, 3, 4))
    state = run.state()
    for i, c in enumerate((1, 2)):
        BM.assert_matches(got, i, tab[c]["sel"][key])
        assert np.array_equal(state[c], tab[c]["sel"][key]["best_plan"])
    run.close()


# ---- 4. continuation ---------------------------------------------------------------------------------
def _valid_plan(g, spec, a, k, lo, hi):
    pops = np.bincount(a, weights=spec.pop.astype(np.int64), minlength=k)
    return lo <= pops.min() and pops.max() <= hi and all(
        len(np.nonzero(a == d)[0]) > 0 and nx.is_connected(g.subgraph(np.nonzero(a == d)[0])) for d in range(k))


def test_continuation(gpu):
    """Twin runs: A rewinds after 40 steps, B does not, both run 20 more.  A chain whose best is the
    window's end continues exactly as B's; every other continues as a valid ReCom chain from the
    restored plan.  A checkpoint taken after the rewind resumes bit for bit."""
    case = RC.BY_NAME["reject 8x8 k=4"]
    spec, k = case.spec, case.k
    tab = table(case.name)
    cap = case.steps * spec.n
    A, B = _run(case, cap, trace=True), _run(case, cap, trace=True)
    for r in (A, B):
        r.set_elections(cols_of(case), [(0, 1)])
        r.steps(case.steps)
    len_b = B.stats()["events"].copy()
    A.burst_select(_dev(METRICS["count"]), rewind=True)
    A.trace_reset()
    restored = A.state()
    blob = A.checkpoint()
    A.steps(20)
    B.steps(20)
    sa, sb, fa, fb = A.stats(), B.stats(), A.state(), B.state()
    g = nx.Graph()
    g.add_nodes_from(range(spec.n))
    edges = spec.edges()
    g.add_edges_from(edges.tolist())
    at_end = [c for c, ch in enumerate(tab) if ch["sel"]["count"]["best_t"] == case.steps]
    assert at_end and len(at_end) < case.n_chains
    for c in range(case.n_chains):
        ea = A.events(c)
        if c in at_end:
            assert np.array_equal(fa[c], fb[c])
            for f in STAT_FIELDS:
                if f not in WINDOW:
                    assert sa[f][c] == sb[f][c], (f, c)
            assert ea.tobytes() == B.events(c)[int(len_b[c]):].tobytes()
            continue
        lo, hi = case.chain_bounds(c)
        assert np.array_equal(restored[c], tab[c]["sel"]["count"]["best_plan"])
        S, cut, nb = BM.states_from_events(restored[c], ea, case.steps, case.steps + 20, sa["series_cut0"][c],
                                           sa["series_nb0"][c])
        assert np.array_equal(S[-1], fa[c]) and len(S) == 21
        for a, x, y in zip(S, cut, nb):
            assert _valid_plan(g, spec, a, k, lo, hi)
            assert (x, y) == G.cut_and_boundary(spec, a)[:2]
        u, v = edges[A.recom_trace(c)["edge"][0]]
        assert restored[c][u] != restored[c][v]
    third = _run(case, cap, trace=True)
    third.restore(blob)
    third.steps(20)
    st = third.stats()
    assert np.array_equal(third.state(), fa)
    for f in STAT_FIELDS:
        assert np.array_equal(st[f], sa[f]), f
    for c in range(case.n_chains):
        assert third.events(c).tobytes() == A.events(c).tobytes()
    for r in (A, B, third):
        r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------
def test_refusals(gpu):
    case = RC.BY_NAME["size 8x8 k=4"]
    run = _run(case, 40)
    run.steps(case.steps)
    assert (run.stats()["events"] > 40).all()
    snap = _snapshot(run)
    cut = _dev(METRICS["cut"])
    with pytest.raises(ValueError, match="chain [0-9]+ overflowed"):
        run.burst_select(cut, rewind=True, plans=True)
    with pytest.raises(ValueError, match="fc_run_set_elections"):
        run.burst_select(_dev(METRICS["count"]))
    run.set_elections(cols_of(case), [(0, 1)])
    with pytest.raises(ValueError, match="columns below n_cols"):
        run.burst_select(BurstMetric("gap", 0, 2), rewind=True)
    for c0, nc in ((-1, 2), (4, 2), (0, 6)):
        with pytest.raises(ValueError, match="chain range"):
            run.burst_select(cut, rewind=True, c0=c0, nc=nc)
    with pytest.raises(ValueError, match="unknown kind"):
        run.burst_select(BurstMetric(5), rewind=True)
    _assert_unchanged(run, snap)
    run.close()


# ---- 6. the optimiser --------------------------------------------------------------------------------
def _partition():
    g = nx.grid_graph([8, 8])
    rng = np.random.default_rng(4)
    for nd in g.nodes:
        g.nodes[nd].update(population=1, D=int(rng.integers(0, 50)), R=int(rng.integers(0, 50)))
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "E": C.Election("E", {"Dem": "D", "Rep": "R"})}
    return C.Partition(g, {nd: nd[0] // 2 for nd in g.nodes}, ups)


@pytest.mark.parametrize("which", ["count", "gap"])
def test_optimiser(gpu, which):
    part = _partition()
    el = part.updaters["E"]
    metric, maximize = (O.DistrictCount(el, "Dem"), True) if which == "count" else (O.EfficiencyGap(el), False)
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.2, node_repeats=1)
    pb = C.within_percent_of_ideal_population(part, 0.2)
    opt = O.SingleMetricOptimizer(tree, C.Validator([pb]), part, metric, maximize=maximize, n_chains=8, seed=5)
    res = opt.short_bursts(5, 10)
    trace = res["score_trace"]
    assert trace.shape == (10, 8) and res["best_part"].shape == (8, 64)
    d = np.diff(trace, axis=0)
    assert (d >= 0).all() if maximize else (d <= 0).all()
    assert np.array_equal(res["best_score"], trace[-1])
    start = metric(part)
    assert (trace[0] >= start).all() if maximize else (trace[0] <= start).all()
    assert (trace[-1] != start).any()  # some chain improved on the start plan
    spec = opt.cspec.spec
    g = nx.Graph()
    g.add_nodes_from(range(spec.n))
    g.add_edges_from(spec.edges().tolist())
    for c in range(8):
        assert metric(opt.partition(res["best_part"][c])) == int(res["best_score"][c])
        assert _valid_plan(g, spec, res["best_part"][c].astype(np.int64), 4, opt.cspec.pop_lo, opt.cspec.pop_hi)
    flip_part = C.Partition(part.graph, {nd: (1 if nd[0] >= 4 else -1) for nd in part.graph.nodes},
                            dict(part.updaters, base=lambda p: 1.0, b_nodes=C.b_nodes_bi))
    with pytest.raises(NotImplementedError, match="ReCom chains only"):
        O.SingleMetricOptimizer(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, pb]), flip_part,
                                O.CutEdges(), maximize=False)
