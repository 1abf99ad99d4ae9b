"""GPU checks of the compactness series: ``FlipRun.shape_series`` -- the device
replay of the accepted-flip log against node areas, exterior lengths and shared edge lengths -- bit
for bit against the numpy model (tests/shape_model.py) fed with the same run's ``events()``,
window-start states and ``stats()``; every histogram row sums to the window's yields.
``event_cap`` >= steps + 1 everywhere but the overflow case, so no chain is left out."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest

import shape_model as SM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

pytestmark = pytest.mark.gpu

DIAG = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES
I64 = ctypes.POINTER(ctypes.c_int64)


def _make(spec, k, a0, bases, cap, *, pct, seed=17, flags=0, tune=None, diag=DIAG):
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, pct)
    inits = np.stack([a0] * len(bases))
    cfg = RunConfig(k=k, labels=(-1, 1) if k == 2 else tuple(range(k)),
                    proposal=_lib.FC_PROPOSE_BI_SIGN if k == 2 else _lib.FC_PROPOSE_PAIR, seed=seed, pop_lo=lo,
                    pop_hi=hi, diag_mask=diag, event_cap=cap, flags=flags, tune=tune)
    return FlipRun(FlipGraph(spec), inits, cfg, bases=np.asarray(bases, dtype=np.float64)), inits


def _random_shapes(spec, seed=29):
    """(area 0..5, edge_len 0..3, ext 0..2), zeros included"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 6, spec.n).astype(np.int32), rng.integers(0, 4, spec.n_edges).astype(np.int32),
            rng.integers(0, 3, spec.n).astype(np.int32))


def _unit_shapes(spec):
    """area 1, edge_len 1, no exterior (any graph)"""
    return np.ones(spec.n, dtype=np.int32), np.ones(spec.n_edges, dtype=np.int32), None


def _check(run, shapes, starts, c0=0, nc=None, edges=None):
    """Set the shapes (edges: given, or spanning every chain's Q range as the model finds it), read
    chains [c0, c0 + nc) and compare each with the model.  Returns the models."""
    nc = run.n_chains - c0 if nc is None else nc
    area, edge_len, ext = shapes
    if edges is None:
        free = [SM.replay_run(run, c, shapes, [], starts[c]) for c in range(c0, c0 + nc)]
        edges = SM.spanning_edges([m["q_range"] for m in free])
    run.set_shapes(area, edge_len, ext, edges if len(edges) else None)
    got = run.shape_series(c0, nc)
    state = run.state()
    models = []
    for i in range(nc):
        m = SM.replay_run(run, c0 + i, shapes, edges, starts[c0 + i])
        SM.assert_matches(got, i, m, with_hist=bool(len(edges)))
        assert np.array_equal(m["final"], state[c0 + i])
        models.append(m)
    if not len(edges):
        assert "pp_hist" not in got and "pp_min_hist" not in got
    return models


GRID_BASES = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0]


def _grid_run(steps_cap, bases=GRID_BASES):
    spec = G.grid_graph(12, 11)
    assert spec.n == 132
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    run, inits = _make(spec, 2, a0, bases, steps_cap + 1, pct=0.5)
    return spec, run, inits


@functools.lru_cache(maxsize=None)
def _grid_3000():
    spec, run, inits = _grid_run(3000)
    run.steps(3000)
    assert int(run.stats()["events"].min()) > 64
    return spec, run, inits


@pytest.mark.parametrize("weights", ["unit_square", "random"])
def test_grid_k2_neighbours_inside_a_chunk(gpu, weights):
    """n = 132 (no multiple of 64), six bases: flips of neighbouring nodes and repeated nodes
    inside a chunk of 64 events occur in every chain (seed 17, checked with the CPU oracle when the
    case was written), so a replay that resolved labels per chunk would miss them."""
    spec, run, inits = _grid_3000()
    shapes = G.unit_square_shapes(spec) if weights == "unit_square" else _random_shapes(spec)
    ms = _check(run, shapes, inits)
    assert min(m["chunk_neighbours"] for m in ms) > 0 and min(m["chunk_repeats"] for m in ms) > 0
    # the edges (five across each chain's Q range) split every chain's Q values into >= 2 bins
    assert all((m["pp_hist"].sum(axis=0) > 0).sum() >= 2 for m in ms)
    assert len({tuple(m["pp_sum"]) for m in ms}) == len(ms)  # the chains differ
    if weights == "unit_square":
        # no histograms, and the degenerate single edge
        _check(run, shapes, inits, edges=[])
        ms = _check(run, shapes, inits, edges=[ms[0]["q_range"][1]])
        assert all(m["pp_hist"].shape == (2, 2) for m in ms)


def test_chunk_boundaries_and_windows(gpu):
    """Reads at event counts around the chunk size: every chain at 0 events, some chain at 0 while
    others have some, some chain at exactly 64 and at 65, and at 127, 128 and 129 (two chunks and
    the refill of the second one read ahead); then a window reset mid-run, read whole and as a
    sub-range of chains."""
    spec, run, inits = _grid_run(4000)
    shapes = _random_shapes(spec)
    ms = _check(run, shapes, inits)  # before the first launch: one yield, no event
    assert all(m["yields"] == 1 for m in ms)
    want = {"zero": lambda e: e.min() == 0 < e.max(), "full": lambda e: (e == 64).any(), "over": lambda e: (e == 65).any()}
    # a second chunk read ahead that is refilled: the chain at base 1.0 logs an event per step
    want.update({f"at {m}": (lambda e, m=m: (e == m).any()) for m in (127, 128, 129)})
    for _ in range(1500):  # one step per launch: a chain's count grows by at most one
        run.steps(1)
        e = run.stats()["events"]
        for key in [key for key, cond in want.items() if cond(e)]:
            _check(run, shapes, inits)
            del want[key]
        if not want:
            break
    assert not want, f"conditions not met within the launch bound: {sorted(want)}"
    run.steps(700)
    run.series_reset()
    starts = run.state()
    ms = _check(run, shapes, starts)  # a fresh window: one yield
    assert all(m["yields"] == 1 for m in ms)
    run.steps(900)
    st = run.stats()
    assert (st["series_t0"] > 700).all() and (st["events"] > 64).all()
    _check(run, shapes, starts)
    _check(run, shapes, starts, c0=2, nc=3)
    _check(run, shapes, starts, c0=5, nc=1)
    assert run.shape_series(3, 0)["area_now"].shape[0] == 0


def test_sec11_quadrants_k4(gpu, sec11):
    a0 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    run, inits = _make(sec11, 4, a0, [0.3, 1.0, 2.0], 2501, pct=0.1)
    run.steps(2500)
    assert int(run.stats()["events"].min()) > 64
    ms = _check(run, G.unit_square_shapes(sec11), inits)
    assert all(m["yields"] == 2501 for m in ms)
    _check(run, _random_shapes(sec11), inits, c0=1, nc=2)


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
def test_kgt2(gpu, name):
    """k > 2 up to every district lane in use.  The triangular lattice has degree <= 6 (the
    8-slot rows); the Delaunay graph has nodes of degree above 8 (the 16-slot rows)."""
    spec, k, a0 = _kgt2_case(name)
    width = 8 if int(spec.degree().max()) <= 8 else 16
    assert width == (8 if name == "triangular_k8" else 16)
    steps = 1500
    run, inits = _make(spec, k, a0, [0.5, 2.0], steps + 1, pct=0.1, tune={"multi_flip": 1})
    run.steps(steps)
    assert int(run.stats()["events"].min()) > 64
    ms = _check(run, _random_shapes(spec), inits)
    assert all(m["pp_min_hist"].sum() == steps + 1 for m in ms)
    _check(run, _unit_shapes(spec), inits, c0=1, nc=1)


def test_independent_invariants(gpu, sec11):
    """edge_len = 1, ext = 0, area = population, window from yield 0: perimeters are twice the
    plan's cut edges, now and summed over yields, and areas are the district populations."""
    for spec, k, a0, pct in ((G.grid_graph(12, 11), 2, None, 0.5), (sec11, 4, None, 0.1)):
        if k == 2:
            a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
        else:
            a0 = spec.assignment_array(G.quadrant_plan(spec.nodes), [0, 1, 2, 3])
        run, _ = _make(spec, k, a0, [0.5, 1.0, 3.0], 2001, pct=pct)
        run.steps(2000)
        run.set_shapes(spec.pop, np.ones(spec.n_edges, dtype=np.int32))
        got = run.shape_series()
        st = run.stats()
        assert (st["series_t0"] == 0).all() and (got["yields"] == 2001).all()
        assert np.array_equal(got["perim_now"].sum(axis=1), 2 * st["cut"])
        assert np.array_equal(got["perim_sum"].sum(axis=1), 2 * st["sum_cut"])
        assert np.array_equal(got["area_now"], run.pops())


def test_no_interference_and_checkpoint(gpu):
    """The election series reads the same before and after the shapes are set and read; a blob
    taken with shapes set equals, byte for byte, the one taken just before on the same run (one
    run, so that the uninitialised tail of the event log is the same memory both times); a restored
    run needs the shapes again and then reads what the uninterrupted run reads."""
    spec, run, inits = _grid_run(1500)
    shapes = _random_shapes(spec)
    cols = np.random.default_rng(23).integers(0, 2, (spec.n, 2))
    run.set_elections(cols, [(0, 1)], [-20, 0, 20])
    run.steps(800)
    before = run.election_series()
    blob_plain = run.checkpoint()
    run.set_shapes(shapes[0], shapes[1], shapes[2], [100, 1000, 10000])
    run.shape_series()
    after = run.election_series()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    blob = run.checkpoint()
    assert blob == blob_plain
    _, back, _ = _grid_run(1500)
    back.restore(blob)
    with pytest.raises(ValueError, match="fc_run_set_shapes first"):
        back.shape_series()
    back.set_shapes(shapes[0], shapes[1], shapes[2], [100, 1000, 10000])
    for r in (run, back):
        r.steps(700)
    x, y = run.shape_series(), back.shape_series()
    for key in x:
        assert np.array_equal(x[key], y[key]), key
    _check(back, shapes, inits, edges=[100, 1000, 10000])


def test_through_the_chain_api(gpu):
    """MarkovChain.run() with a Compactness updater: ChainResult.shapes equals the model fed by the
    same chain built by hand."""
    g = nx.grid_graph([10, 10])
    rng = np.random.default_rng(41)
    for nd in g.nodes:
        g.nodes[nd].update(population=1, area=int(rng.integers(1, 5)))
        if g.degree[nd] < 4:
            g.nodes[nd]["boundary_perim"] = int(rng.integers(1, 4))
    for e in g.edges:
        g.edges[e]["shared_perim"] = int(rng.integers(0, 3))
    plan = {nd: (1 if nd[0] >= 5 else -1) for nd in g.nodes}
    updaters = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
                "base": lambda p: 1.3, "shape": C.Compactness()}
    part = C.Partition(g, plan, updaters)
    popbound = C.within_percent_of_ideal_population(part, 0.3)
    steps = 1200
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=part, total_steps=steps, seed=9)
    res = mc.run(series=False, corrected=False)
    assert res.shapes is not None and res.rce is None and res.elections is None
    spec = G.from_networkx(g)
    shapes_in = C.Compactness().arrays(g, spec, spec.edges())
    _, (lo, hi) = G.population_bounds(100, 2, 0.3)
    cfg = RunConfig(k=2, labels=(-1, 1), seed=9, base=1.3, pop_lo=lo, pop_hi=hi, diag_mask=DIAG, event_cap=steps)
    run = FlipRun(FlipGraph(spec), spec.assignment_array(plan, [-1, 1])[None, :], cfg)
    run.steps(steps - 1)
    m = _check(run, shapes_in, run._init, edges=[])[0]
    assert res.shapes["yields"] == steps == m["yields"]
    for key in ("area_now", "perim_now", "perim_sum", "pp_now", "pp_sum"):
        assert np.array_equal(res.shapes[key], m[key]), key
    assert res.shapes["pp_min_sum"] == m["pp_min_sum"]
    # the host updater on the initial partition is yield 0; on the final one, the last yield
    first = part["shape"]
    final = C.Partition(g, res.final_assignment, {"shape": C.Compactness()})["shape"]
    for d, lab in enumerate((-1, 1)):
        assert (final[lab]["area"], final[lab]["perimeter"], final[lab]["q"]) == \
            (m["area_now"][d], m["perim_now"][d], m["pp_now"][d])
        assert first[lab]["area"] + first[-lab]["area"] == int(m["area_now"].sum())
    # a chain without the updater leaves the attribute alone
    del updaters["shape"]
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=C.Partition(g, plan, updaters), total_steps=50, seed=9)
    assert mc.run().shapes is None


def test_error_codes(gpu, sec11):
    spec, run, inits = _grid_run(500)
    area, edge_len, ext = _random_shapes(spec)
    run.steps(500)
    with pytest.raises(ValueError, match="fc_run_set_shapes first"):
        run.shape_series()
    neg_a, neg_l, neg_x = area.copy(), edge_len.copy(), ext.copy()
    neg_a[5] = neg_l[7] = neg_x[9] = -1
    big_a, big_l, big_x = area.copy(), edge_len.copy(), ext.copy()
    big_a[:2] = 2 ** 30
    big_l[0], big_x[0] = 2 ** 30 + 2 ** 29, 2 ** 29  # ext and edge_len overflow together, neither alone
    for args in ((neg_a, edge_len, ext), (area, neg_l, ext), (area, edge_len, neg_x), (big_a, edge_len, ext),
                 (area, big_l, big_x), (area, edge_len, ext, [3, 3]), (area, edge_len, ext, [5, 1]),
                 (area, edge_len, ext, list(range(65))), (area[:-1], edge_len, ext), (area, edge_len[:-1], ext)):
        with pytest.raises(ValueError):
            run.set_shapes(*args)
    with pytest.raises(ValueError):  # a failed call sets nothing
        run.shape_series()
    run.set_shapes(area, edge_len, ext, list(range(64)))  # 64 edges are allowed
    run.set_shapes(area, edge_len)
    for c0, nc in ((-1, 2), (0, 7), (6, 1), (2, -1)):
        with pytest.raises(ValueError, match="chain range"):
            run.shape_series(c0, nc)
    # histograms asked for without edges (the Python reader never does: the raw call)
    L = _lib.load()
    buf = np.zeros(64, dtype=np.int64)
    for pos in (6, 7):
        ptrs = [None] * 8
        ptrs[pos] = buf.ctypes.data_as(I64)
        assert L.fc_run_shape_series(run.handle, 0, 1, *ptrs) == _lib.FC_ERR_ARG and b"pp_edges" in L.fc_last_error()
    assert L.fc_run_shape_series(run.handle, 0, 6, *([None] * 8)) == _lib.FC_OK
    # no FC_DIAG_SERIES
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    plain, _ = _make(spec, 2, a0, [1.0], 0, pct=0.5, diag=_lib.FC_DIAG_WAIT)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.set_shapes(area, edge_len, ext)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.shape_series()
    # an overflowed log is an argument error that names the chain
    small, _ = _make(spec, 2, a0, [0.2, 1.0], 40, pct=0.5)
    small.set_shapes(area, edge_len, ext)
    small.steps(600)
    ev = small.stats()["events"]
    assert ev[1] > 40
    with pytest.raises(ValueError, match=f"chain {0 if ev[0] > 40 else 1} overflowed event_cap"):
        small.shape_series()
    # a ReCom run has no flip log
    a4 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    _, (lo, hi) = G.population_bounds(sec11.n, 4, 0.1)
    cfg = RunConfig(k=4, labels=(0, 1, 2, 3), proposal=_lib.FC_PROPOSE_RECOM, seed=3, pop_lo=lo, pop_hi=hi,
                    diag_mask=0, recom_pop_target=sec11.n / 4, recom_epsilon=0.1)
    recom = FlipRun(FlipGraph(sec11), a4[None, :], cfg)
    with pytest.raises(NotImplementedError):
        recom.set_shapes(*G.unit_square_shapes(sec11)[:2])
    with pytest.raises(NotImplementedError):
        recom.shape_series()
    # a chain image beyond the LDS limit: 28,900 nodes (the event log's 16-bit |cut| bounds a run's
    # edges by 65,535), k = 32 and 64 edges (33 rows of 65 bins)
    big = G.grid_graph(170, 170)
    plan = G.strip_plan(big, 32)
    wide, _ = _make(big, 32, big.assignment_array(plan, list(range(32))), [1.0], 8, pct=0.5)
    with pytest.raises(NotImplementedError, match="48 KB of LDS"):
        wide.set_shapes(np.ones(big.n, dtype=np.int32), np.ones(big.n_edges, dtype=np.int32), None, list(range(64)))
    wide.set_shapes(np.ones(big.n, dtype=np.int32), np.ones(big.n_edges, dtype=np.int32))  # fits without them
