"""GPU checks of the election series: ``FlipRun.election_series`` -- the device
replay of the accepted-flip log against node vote columns -- bit for bit against the numpy model
(tests/election_model.py) fed with the same run's ``events()``, window-start states and
``stats()``; ``tally_now`` also against tallies of ``run.state()``; every histogram row sums to
the window's yields.  ``event_cap`` >= steps + 1 everywhere but the overflow case, so no chain is
left out."""
import functools

import networkx as nx
import numpy as np
import pytest

import election_model as EM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

pytestmark = pytest.mark.gpu

DIAG = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES


def _make(spec, k, a0, bases, cap, *, pct, seed=17, flags=0, tune=None, diag=DIAG):
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, pct)
    inits = np.stack([a0] * len(bases))
    cfg = RunConfig(k=k, labels=(-1, 1) if k == 2 else tuple(range(k)),
                    proposal=_lib.FC_PROPOSE_BI_SIGN if k == 2 else _lib.FC_PROPOSE_PAIR, seed=seed, pop_lo=lo,
                    pop_hi=hi, diag_mask=diag, event_cap=cap, flags=flags, tune=tune)
    return FlipRun(FlipGraph(spec), inits, cfg, bases=np.asarray(bases, dtype=np.float64)), inits


def _votes(n, n_cols, seed=23, top=2):
    return np.random.default_rng(seed).integers(0, top, (n, n_cols)).astype(np.int64)


def _check(run, cols, elections, starts, c0=0, nc=None, edges=None):
    """Set the elections (edges: given, or spanning every chain's gap range as the model finds
    it), read chains [c0, c0 + nc) and compare each with the model.  Returns the models."""
    nc = run.n_chains - c0 if nc is None else nc
    if edges is None:
        free = [EM.replay_run(run, c, cols, elections, [], starts[c]) for c in range(c0, c0 + nc)]
        edges = EM.spanning_edges([r for m in free for r in m.get("gap_range", [])]) if elections else []
    run.set_elections(cols, elections, edges if len(edges) else None)
    got = run.election_series(c0, nc)
    state = run.state()
    models = []
    for i in range(nc):
        m = EM.replay_run(run, c0 + i, cols, elections, edges, starts[c0 + i])
        EM.assert_matches(got, i, m, with_hist=bool(len(edges)) and bool(elections))
        assert np.array_equal(m["final"], state[c0 + i])
        now = np.zeros_like(m["tally_now"])
        np.add.at(now, state[c0 + i].astype(np.int64), cols)
        assert np.array_equal(got["tally_now"][i], now)
        models.append(m)
    if not len(edges):
        assert "gap_hist" not in got
    return models


GRID_BASES = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
EL8 = [(0, 1), (7, 2), (3, 0), (5, 6)]


def _grid_run(steps_cap, flags=0):
    spec = G.grid_graph(12, 11)
    assert spec.n == 132
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    run, inits = _make(spec, 2, a0, GRID_BASES, steps_cap + 1, pct=0.5, flags=flags)
    return spec, run, inits


@pytest.mark.parametrize("global_cur", [False, True])
def test_grid_k2_ties_and_chunk_repeats(gpu, global_cur):
    """n = 132 (no multiple of 64), 0/1 votes: tied districts and nodes repeated inside a chunk
    of 64 events are frequent.  2 columns, then 8 with 4 elections, then 3 (the 4-column
    instance); the current assignment in LDS and in a global row."""
    steps = 3000
    spec, run, inits = _grid_run(steps, _lib.FC_FLAG_VOTES_GLOBAL_CUR if global_cur else 0)
    run.steps(steps)
    assert int(run.stats()["events"].min()) > 64
    ms = _check(run, _votes(spec.n, 2), [(0, 1)], inits)
    # the case keeps its point: both do occur, and the chains differ
    assert sum(m["ties"] for m in ms) > 0 and min(m["chunk_repeats"] for m in ms) > 0
    assert len({tuple(m["seats_hist"].ravel()) for m in ms}) > 1
    ms = _check(run, _votes(spec.n, 8), EL8, inits)
    assert sum(m["ties"] for m in ms) > 0
    assert all((m["gap_hist"] > 0).sum(axis=1).min() >= 2 for m in ms)  # the edges split the gap ranges
    _check(run, _votes(spec.n, 3, top=50), [(2, 0), (1, 2)], inits)
    # the degenerate single edge, and tallies only
    ms = _check(run, _votes(spec.n, 2), [(1, 0)], inits, edges=[0])
    assert all(m["gap_hist"].shape == (1, 2) for m in ms)
    _check(run, _votes(spec.n, 5, top=1000), [], inits)


def test_chunk_boundaries_and_windows(gpu):
    """Reads at event counts around the chunk size: every chain at 0 events, some chain at 0 while
    others have some, some chain at exactly 64 and at 65; then a window reset mid-run, read whole
    and as a sub-range of chains."""
    spec, run, inits = _grid_run(4000)
    cols, el = _votes(spec.n, 2), [(0, 1)]
    ms = _check(run, cols, el, inits)  # before the first launch: one yield, no event
    assert all(m["yields"] == 1 for m in ms)
    want = {"zero": lambda e: e.min() == 0 < e.max(), "full": lambda e: (e == 64).any(), "over": lambda e: (e == 65).any()}
    for _ in range(1500):  # one step per launch: a chain's count grows by at most one
        run.steps(1)
        e = run.stats()["events"]
        for key in [key for key, cond in want.items() if cond(e)]:
            _check(run, cols, el, inits)
            del want[key]
        if not want:
            break
    assert not want, f"conditions not met within the launch bound: {sorted(want)}"
    run.steps(700)
    run.series_reset()
    starts = run.state()
    ms = _check(run, cols, el, starts)  # a fresh window: one yield
    assert all(m["yields"] == 1 for m in ms)
    run.steps(900)
    st = run.stats()
    assert (st["series_t0"] > 700).all() and (st["events"] > 64).all()
    _check(run, cols, el, starts)
    _check(run, cols, el, starts, c0=2, nc=3)
    _check(run, cols, el, starts, c0=5, nc=1)
    assert run.election_series(3, 0)["tally_now"].shape[0] == 0


def test_sec11_launch_split(gpu, sec11):
    """sec11 with the reference's labels (-1, 1): the same 6000 steps in 1 and in 4 launches."""
    a0 = sec11.assignment_array(G.sec11_plan(0, sec11.nodes), [-1, 1])
    bases = [0.1, 1 / G.SEC11_MU, 1.0, G.SEC11_MU]
    cols = _votes(sec11.n, 4, top=30)
    el = [(0, 1), (2, 3)]
    outs = []
    for launches in (1, 4):
        run, inits = _make(sec11, 2, a0, bases, 6001, pct=0.1)
        for _ in range(launches):
            run.steps(6000 // launches)
        _check(run, cols, el, inits)
        outs.append(run.election_series())
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key]), key


@functools.lru_cache(maxsize=None)
def _kgt2_case(name):
    if name == "triangular_k8":
        spec, k = G.triangular_graph(30, 58), 8
        plan = G.strip_plan(spec, k)
    else:
        spec, k = G.delaunay_graph(2000, seed=0), int(name.rsplit("k", 1)[1])
        plan = G.bisection_plan(spec, k)
    return spec, k, spec.assignment_array(plan, list(range(k)))


@pytest.mark.parametrize("name", ["triangular_k8", "delaunay_k18", "delaunay_k32"])
def test_kgt2_multi_flip(gpu, name):
    """k > 2 (the old district of an event comes from the replayed assignment), with the
    multi-flip commit on; k = 32 has every district lane in use (it is beyond the district-graph
    rule, so the setting has no effect there and flips commit one at a time)."""
    spec, k, a0 = _kgt2_case(name)
    steps = 4000 if name == "triangular_k8" else 2500
    run, inits = _make(spec, k, a0, [0.5, 1.0, 2.0, 4.0], steps + 1, pct=0.1, tune={"multi_flip": 1})
    run.steps(steps)
    if k <= 31:
        assert run.kernel_name().endswith((", true, 1>", ", true, 2>"))  # a multi-flip instance
    assert int(run.stats()["events"].min()) > 64
    ms = _check(run, _votes(spec.n, 8, top=3), EL8, inits)
    assert all(m["seats_hist"].sum(axis=1).tolist() == [steps + 1] * 4 for m in ms)
    _check(run, _votes(spec.n, 2, top=100), [(0, 1)], inits, c0=1, nc=2)


def test_frank_k2(gpu, frank):
    assert frank.n == 800
    a0 = frank.assignment_array(G.frank_plan(1, frank.nodes), [-1, 1])
    run, inits = _make(frank, 2, a0, [0.3, 1.0, 1 / 0.3], 2001, pct=0.5)
    run.steps(2000)
    _check(run, _votes(frank.n, 2), [(0, 1)], inits)
    _check(run, _votes(frank.n, 6, top=20), [(4, 5), (0, 3), (1, 2)], inits)


def test_checkpoint_does_not_hold_the_columns(gpu):
    """Columns are not trajectory state: a blob has the same size with and without them (the
    unused tail of the event log is uninitialised memory, so sizes are compared, not bytes), it
    restores into a run that never had columns, and the restored run reads the same series once
    it has been given them."""
    spec, run, inits = _grid_run(1500)
    _, plain, _ = _grid_run(1500)
    cols, el = _votes(spec.n, 2), [(0, 1)]
    run.set_elections(cols, el, [-20, 0, 20])
    for r in (run, plain):
        r.steps(800)
    blob = run.checkpoint()
    assert len(blob) == len(plain.checkpoint())
    _, back, _ = _grid_run(1500)
    back.restore(blob)
    with pytest.raises(ValueError, match="fc_run_set_elections first"):
        back.election_series()
    back.set_elections(cols, el, [-20, 0, 20])
    for r in (run, back):
        r.steps(700)
    a, b = run.election_series(), back.election_series()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    _check(back, cols, el, inits, edges=[-20, 0, 20])


def test_through_the_chain_api(gpu):
    """MarkovChain.run() with Election updaters: ChainResult.elections equals
    FlipRun.election_series of chain 0 of the same chain built by hand."""
    g = nx.grid_graph([10, 10])
    rng = np.random.default_rng(41)
    for nd in g.nodes:
        g.nodes[nd].update(population=1, D=int(rng.integers(0, 5)), R=int(rng.integers(0, 5)), G=int(rng.integers(0, 2)))
    plan = {nd: (1 if nd[0] >= 5 else -1) for nd in g.nodes}
    updaters = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
                "base": lambda p: 1.3, "E1": C.Election("E1", {"Dem": "D", "Rep": "R"}),
                "E2": C.Election("E2", {"Green": "G", "Dem": "D"})}
    part = C.Partition(g, plan, updaters)
    assert part["E1"].seats("Dem") + part["E1"].seats("Rep") <= 2
    popbound = C.within_percent_of_ideal_population(part, 0.3)
    steps = 1200
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=part, total_steps=steps, seed=9)
    res = mc.run(series=False, corrected=False)
    assert set(res.elections) == {"E1", "E2"} and res.rce is None
    spec = G.from_networkx(g, columns=("D", "R", "G"))
    cols = np.stack([spec.columns[c] for c in ("D", "R", "G")], axis=1)
    _, (lo, hi) = G.population_bounds(100, 2, 0.3)
    cfg = RunConfig(k=2, labels=(-1, 1), seed=9, base=1.3, pop_lo=lo, pop_hi=hi, diag_mask=DIAG, event_cap=steps)
    run = FlipRun(FlipGraph(spec), spec.assignment_array(plan, [-1, 1])[None, :], cfg)
    run.steps(steps - 1)
    _check(run, cols, [(0, 1), (2, 0)], run._init, edges=[])
    es = run.election_series()
    for e, (key, ja, jb) in enumerate((("E1", 0, 1), ("E2", 2, 0))):
        r = res.elections[key]
        assert r["yields"] == steps == int(es["yields"][0])
        assert np.array_equal(r["seats_hist"], es["seats_hist"][0, e]) and r["seats_hist"].sum() == steps
        assert np.array_equal(r["wins_sum"], es["wins_sum"][0, e])
        assert r["gap_sum"] == int(es["gap_sum"][0, e])
        assert np.array_equal(r["tally_sum"], es["tally_sum"][0][:, [ja, jb]])
    assert res.elections["E1"]["parties"] == ["Dem", "Rep"] and res.elections["E2"]["columns"] == ["G", "D"]
    # a chain without Election updaters leaves the attribute alone
    del updaters["E1"], updaters["E2"]
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=C.Partition(g, plan, updaters), total_steps=50, seed=9)
    assert mc.run().elections is None


def test_error_codes(gpu, sec11):
    spec, run, inits = _grid_run(500)
    cols = _votes(spec.n, 2)
    run.steps(500)
    with pytest.raises(ValueError, match="fc_run_set_elections first"):
        run.election_series()
    bad = cols.copy()
    bad[5, 1] = -1
    big = cols.copy()
    big[:2, 0] = 2 ** 30
    for args in ((bad, [(0, 1)]), (big, [(0, 1)]), (cols, [(0, 2)]), (cols, [(-1, 0)]), (cols, [(1, 1)]),
                 (cols, [(0, 1)], [3, 3]), (cols, [(0, 1)], [5, 1]), (cols, [(0, 1)] * 5),
                 (_votes(spec.n, 9), [(0, 1)]), (cols, [(0, 1)], list(range(257)))):
        with pytest.raises(ValueError):
            run.set_elections(*args)
    with pytest.raises(ValueError):  # a failed call sets nothing
        run.election_series()
    run.set_elections(cols, [(0, 1)])
    for c0, nc in ((-1, 2), (0, 7), (6, 1), (2, -1)):
        with pytest.raises(ValueError, match="chain range"):
            run.election_series(c0, nc)
    # gap_hist asked for without edges (the Python reader never does: the raw call)
    import ctypes
    buf = np.zeros(64, dtype=np.int64)
    rc = _lib.load().fc_run_election_series(run.handle, 0, 1, None, None, None, None, None,
                                            buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == _lib.FC_ERR_ARG and b"gap_edges" in _lib.load().fc_last_error()
    assert _lib.load().fc_run_election_series(run.handle, 0, 6, None, None, None, None, None, None) == _lib.FC_OK
    # no FC_DIAG_SERIES
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    plain, _ = _make(spec, 2, a0, [1.0], 0, pct=0.5, diag=_lib.FC_DIAG_WAIT)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.set_elections(cols, [(0, 1)])
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.election_series()
    # an overflowed log is an argument error that names the chain
    small, _ = _make(spec, 2, a0, [0.2, 1.0], 40, pct=0.5)
    small.set_elections(cols, [(0, 1)])
    small.steps(600)
    ev = small.stats()["events"]
    assert ev[1] > 40
    with pytest.raises(ValueError, match=f"chain {0 if ev[0] > 40 else 1} overflowed event_cap"):
        small.election_series()
    # a ReCom run has no flip log
    a4 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    _, (lo, hi) = G.population_bounds(sec11.n, 4, 0.1)
    cfg = RunConfig(k=4, labels=(0, 1, 2, 3), proposal=_lib.FC_PROPOSE_RECOM, seed=3, pop_lo=lo, pop_hi=hi,
                    diag_mask=0, recom_pop_target=sec11.n / 4, recom_epsilon=0.1)
    recom = FlipRun(FlipGraph(sec11), a4[None, :], cfg)
    with pytest.raises(NotImplementedError):
        recom.set_elections(_votes(sec11.n, 2), [(0, 1)])
    with pytest.raises(NotImplementedError):
        recom.election_series()
