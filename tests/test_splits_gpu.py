"""GPU checks of the locality-splits series: ``FlipRun.split_series`` -- the device
replay of the accepted-flip log against a node labelling -- bit for bit against the numpy model
(tests/split_model.py) fed with the same run's ``events()``, window-start states and ``stats()``,
and the invariants that tie the outputs together, on the device's numbers.  ``event_cap`` >=
steps + 1 everywhere but the overflow case, so no chain is left out."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest

import split_model as SM
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


def _check(run, node_loc, starts, c0=0, nc=None):
    """Set the labelling, read chains [c0, c0 + nc) and compare each with the model; the invariants
    on the model's numbers and on the device's.  Returns the models."""
    nc = run.n_chains - c0 if nc is None else nc
    n, n_loc = run.graph.n, int(np.max(node_loc)) + 1
    run.set_localities(node_loc)
    got = run.split_series(c0, nc)
    state = run.state()
    # cells_now summed over the localities is pops() where every node has population 1
    pops = run.pops() if (run.graph.spec.pop == 1).all() else [None] * run.n_chains
    models = []
    for i in range(nc):
        m = SM.replay_run(run, c0 + i, node_loc, starts[c0 + i])
        SM.assert_matches(got, i, m)
        assert np.array_equal(m["final"], state[c0 + i])
        SM.check_invariants(m, n_loc, n, pops=pops[c0 + i])
        SM.check_invariants({key: (val if key == "x_max" else val[i]) for key, val in got.items()}, n_loc, n,
                            pops=pops[c0 + i])
        models.append(m)
    return models


def _bands(spec, nx_, ny_):
    """Localities by coordinate bands: nx_ x ny_ equal-count bands of the node positions, the
    occupied ones numbered densely."""
    def band(x, m):
        return np.searchsorted(np.quantile(x, np.arange(1, m) / m), x, side="right")
    raw = band(spec.pos[:, 0], nx_) * ny_ + band(spec.pos[:, 1], ny_)
    return np.unique(raw, return_inverse=True)[1].astype(np.int32)


GRID_BASES = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0]


def _grid_run(steps_cap, bases=GRID_BASES):
    spec = G.grid_graph(12, 11)
    assert spec.n == 132 and (spec.pop == 1).all()
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    run, inits = _make(spec, 2, a0, bases, steps_cap + 1, pct=0.5)
    return spec, run, inits


@functools.lru_cache(maxsize=None)
def _grid_3000():
    spec, run, inits = _grid_run(3000)
    run.steps(3000)
    assert int(run.stats()["events"].min()) > 64
    return spec, run, inits


def test_grid_k2_blocks(gpu):
    """n = 132 (no multiple of 64), six bases, 2 x 3 blocks (24 localities, none split at the
    start): cells reach and leave 0, and events on one locality share a chunk of 64, in every
    chain.  The totals are those of the CPU oracle for exactly these inputs."""
    spec, run, inits = _grid_3000()
    loc = G.block_localities(spec, 2, 3)
    assert int(loc.max()) + 1 == 24
    assert SM.aggregates(SM.cell_table(inits[0].astype(np.int64), loc, 24, 2))[1] == 0
    ms = _check(run, loc, inits)
    for m in ms:
        assert m["crossings"] > 0 and m["chunk_same_loc"] > 0
        assert (m["splits_hist"] > 0).sum() >= 2 and (m["excess_hist"] > 0).sum() >= 2
    assert sum(m["crossings"] for m in ms) >= 178 and sum(m["chunk_same_loc"] for m in ms) >= 967
    assert len(set(np.concatenate([m["splits_values"] for m in ms]).tolist())) >= 9
    assert len({tuple(m["parts_sum"]) for m in ms}) == len(ms)  # the chains differ


@pytest.mark.parametrize("labelling", ["columns", "one", "nodes"])
def test_grid_k2_other_labellings(gpu, labelling):
    spec, run, inits = _grid_3000()
    loc = {"columns": G.block_localities(spec, 1, 11), "one": np.zeros(spec.n, dtype=np.int32),
           "nodes": np.arange(spec.n, dtype=np.int32)}[labelling]
    ms = _check(run, loc, inits)
    got = run.split_series()
    if labelling == "one":
        assert got["x_max"] == 1 and got["splits_hist"].shape == (6, 2) and got["excess_hist"].shape == (6, 2)
        assert (got["splits_hist"][:, 1] == got["yields"]).all()  # both districts always hold nodes
    if labelling == "nodes":
        assert got["x_max"] == 0 and got["excess_hist"].shape == (6, 1)
        assert (got["splits_hist"][:, 0] == got["yields"]).all() and (got["sq_sum"] == spec.n * got["yields"]).all()
        assert all(m["crossings"] == 2 * int(e) for m, e in zip(ms, run.stats()["events"]))


def test_chunk_boundaries_and_windows(gpu):
    """Reads at event counts around the chunk size: every chain at 0 events, some chain at 0 while
    others have some, some chain at exactly 64 and at 65; then a window reset mid-run, read whole
    and as sub-ranges of chains, and nc = 0."""
    spec, run, inits = _grid_run(4000)
    loc = G.block_localities(spec, 2, 3)
    ms = _check(run, loc, inits)  # before the first launch: one yield, no event
    assert all(m["yields"] == 1 for m in ms)
    want = {"zero": lambda e: e.min() == 0 < e.max(), "full": lambda e: (e == 64).any(), "over": lambda e: (e == 65).any()}
    for _ in range(1500):  # one step per launch: a chain's count grows by at most one
        run.steps(1)
        e = run.stats()["events"]
        for key in [key for key, cond in want.items() if cond(e)]:
            _check(run, loc, inits)
            del want[key]
        if not want:
            break
    assert not want, f"conditions not met within the launch bound: {sorted(want)}"
    run.steps(700)
    run.series_reset()
    starts = run.state()
    ms = _check(run, loc, starts)  # a fresh window: one yield
    assert all(m["yields"] == 1 for m in ms)
    run.steps(900)
    st = run.stats()
    assert (st["series_t0"] > 700).all() and (st["events"] > 64).all()
    _check(run, loc, starts)
    _check(run, loc, starts, c0=2, nc=3)
    _check(run, loc, starts, c0=5, nc=1)
    empty = run.split_series(3, 0)
    assert empty["cells_now"].shape == (0, 24, 2) and empty["splits_now"].shape == (0,)


def test_grid_quadrants_k4(gpu):
    """12 x 12 grid, quadrant plan, PAIR proposals, 3 x 3 blocks (16 localities).  The totals are
    those of the CPU oracle for exactly these inputs."""
    spec = G.grid_graph(12, 12)
    a0 = spec.assignment_array(G.quadrant_plan(spec.nodes, 6), [0, 1, 2, 3])
    run, inits = _make(spec, 4, a0, [0.3, 1.0, 2.0], 2501, pct=0.5)
    run.steps(2500)
    assert int(run.stats()["events"].min()) > 64
    loc = G.block_localities(spec, 3, 3)
    assert int(loc.max()) + 1 == 16
    ms = _check(run, loc, inits)
    assert all(m["yields"] == 2501 for m in ms)
    assert sum(m["crossings"] for m in ms) >= 166 and sum(m["chunk_same_loc"] for m in ms) >= 909
    _check(run, G.block_localities(spec, 1, 12), inits, c0=1, nc=2)


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
    """k > 2 up to every district in use, localities by coordinate bands (12 x 9 of them)."""
    spec, k, a0 = _kgt2_case(name)
    steps = 1500
    run, inits = _make(spec, k, a0, [0.5, 2.0], steps + 1, pct=0.1, tune={"multi_flip": 1})
    run.steps(steps)
    assert int(run.stats()["events"].min()) > 64
    loc = _bands(spec, 12, 9)
    assert 64 < int(loc.max()) + 1 <= 108
    ms = _check(run, loc, inits)
    assert all(m["splits_hist"].sum() == steps + 1 and m["crossings"] > 0 for m in ms)
    _check(run, _bands(spec, 3, 1), inits, c0=1, nc=1)


def test_excess_hist_clamp(gpu, sec11):
    """sec11, k = 4.  2 x 1 blocks: 800 localities, x_max = 1596 - 800 = 796, so X = x_max.
    4 x 1 blocks: 400 localities, x_max = 1196 > 1023, so X = 1023 and the top bin stands for every
    larger excess."""
    a0 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    run, inits = _make(sec11, 4, a0, [0.3, 1.0, 2.0], 2501, pct=0.1)
    run.steps(2500)
    for bx, n_loc, x_max in ((2, 800, 796), (4, 400, 1196)):
        loc = G.block_localities(sec11, bx, 1)
        assert int(loc.max()) + 1 == n_loc and SM.x_max_of(loc, n_loc, 4) == x_max
        ms = _check(run, loc, inits)
        got = run.split_series()
        assert got["x_max"] == x_max and got["excess_hist"].shape == (3, min(x_max, 1023) + 1)
        assert all(m["crossings"] > 0 for m in ms)


def test_interleaving_replacement_and_checkpoint(gpu):
    """The election and compactness series read the same before and after the labelling is set and
    read; a second labelling replaces the first; a blob taken with a labelling set equals, byte for
    byte, the one taken just before on the same run; a restored run needs the labelling again and
    then reads what the uninterrupted run reads."""
    spec, run, inits = _grid_run(1500)
    cols = np.random.default_rng(23).integers(0, 2, (spec.n, 2))
    run.set_elections(cols, [(0, 1)], [-20, 0, 20])
    run.set_shapes(*G.unit_square_shapes(spec), [100, 1000, 10000])
    run.steps(800)
    before = run.election_series(), run.shape_series()
    blob_plain = run.checkpoint()
    blocks, columns = G.block_localities(spec, 2, 3), G.block_localities(spec, 1, 12)
    first = _check(run, blocks, inits)
    after = run.election_series(), run.shape_series()
    for x, y in zip(before, after):
        for key in x:
            assert np.array_equal(x[key], y[key]), key
    second = _check(run, columns, inits)  # replaced: 11 localities now
    assert run.split_series()["split_sum"].shape == (6, 11)
    assert first[0]["split_sum"].shape != second[0]["split_sum"].shape
    again = _check(run, blocks, inits, c0=1, nc=4)  # and back, on a sub-range
    assert np.array_equal(again[0]["parts_sum"], first[1]["parts_sum"])
    blob = run.checkpoint()
    assert blob == blob_plain
    _, back, _ = _grid_run(1500)
    back.restore(blob)
    with pytest.raises(ValueError, match="fc_run_set_localities first"):
        back.split_series()
    back.set_localities(blocks)
    run.set_localities(blocks)
    for r in (run, back):
        r.steps(700)
    x, y = run.split_series(), back.split_series()
    for key in x:
        assert np.array_equal(x[key], y[key]), key
    _check(back, blocks, inits)


def test_through_the_chain_api(gpu):
    """MarkovChain.run() with a LocalitySplits updater: ChainResult.splits equals the model fed by
    the same chain built by hand."""
    g = nx.grid_graph([10, 10])
    for nd in g.nodes:
        g.nodes[nd].update(population=1, county=f"c{nd[0] // 3}{nd[1] // 4}")
    plan = {nd: (1 if nd[0] >= 5 else -1) for nd in g.nodes}
    updaters = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
                "base": lambda p: 1.3, "splits": C.LocalitySplits()}
    part = C.Partition(g, plan, updaters)
    popbound = C.within_percent_of_ideal_population(part, 0.3)
    steps = 1200
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=part, total_steps=steps, seed=9)
    res = mc.run(series=False, corrected=False)
    assert res.splits is not None and res.rce is None and res.shapes is None and res.elections is None
    spec = G.from_networkx(g)
    labels, node_loc = C.LocalitySplits().arrays(g, spec)
    assert res.splits["localities"] == labels and len(labels) == 12
    _, (lo, hi) = G.population_bounds(100, 2, 0.3)
    cfg = RunConfig(k=2, labels=(-1, 1), seed=9, base=1.3, pop_lo=lo, pop_hi=hi, diag_mask=DIAG, event_cap=steps)
    run = FlipRun(FlipGraph(spec), spec.assignment_array(plan, [-1, 1])[None, :], cfg)
    run.steps(steps - 1)
    m = _check(run, node_loc, run._init)[0]
    assert res.splits["yields"] == steps == m["yields"] and m["crossings"] > 0
    for key in SM.ARRAYS:
        assert np.array_equal(res.splits[key], m[key]), key
    for key in SM.SCALARS + ("x_max",):
        assert res.splits[key] == m[key], key
    # the host updater on the initial partition is yield 0; on the final one, the last yield
    final = C.Partition(g, res.final_assignment, {"splits": C.LocalitySplits()})["splits"]
    assert final["num_split"] == m["splits_now"] and final["excess"] == m["excess_now"]
    assert [final[lab]["parts"] for lab in labels] == m["parts_now"].tolist()
    assert m["splits_hist"][part["splits"]["num_split"]] > 0
    # a chain without the updater leaves the attribute alone
    del updaters["splits"]
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                       accept=C.cut_accept, initial_state=C.Partition(g, plan, updaters), total_steps=50, seed=9)
    assert mc.run().splits is None


def test_error_codes(gpu, sec11):
    spec, run, inits = _grid_run(500)
    loc = G.block_localities(spec, 2, 3)
    run.steps(500)
    with pytest.raises(ValueError, match="fc_run_set_localities first"):
        run.split_series()
    low, high, gap = loc.copy(), loc.copy(), loc.copy()
    low[5], high[7] = -1, 24
    gap[gap == 3] = 2  # label 3 unused
    for bad in (low, gap, loc[:-1], loc.astype(np.float64)):
        with pytest.raises(ValueError):
            run.set_localities(bad)
    L = _lib.load()
    ptr = np.ascontiguousarray(loc).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for n_loc in (0, -3, 23, spec.n + 1):  # 23: label 23 out of range
        assert L.fc_run_set_localities(run.handle, n_loc, ptr) == _lib.FC_ERR_ARG
    hp = np.ascontiguousarray(high).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.fc_run_set_localities(run.handle, 24, hp) == _lib.FC_ERR_ARG and b"out of range" in L.fc_last_error()
    assert L.fc_run_set_localities(run.handle, 24, None) == _lib.FC_ERR_ARG
    with pytest.raises(ValueError):  # a failed call sets nothing
        run.split_series()
    run.set_localities(loc)
    for c0, nc in ((-1, 2), (0, 7), (6, 1), (2, -1)):
        with pytest.raises(ValueError, match="chain range"):
            run.split_series(c0, nc)
    assert L.fc_run_split_series(run.handle, 0, 6, *([None] * 7)) == _lib.FC_OK  # any output may be NULL
    buf = np.zeros(6, dtype=np.int64)
    ptrs = [None] * 7
    ptrs[4] = buf.ctypes.data_as(I64)
    assert L.fc_run_split_series(run.handle, 0, 6, *ptrs) == _lib.FC_OK
    assert np.array_equal(buf, run.split_series()["sq_sum"])
    # no FC_DIAG_SERIES
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    plain, _ = _make(spec, 2, a0, [1.0], 0, pct=0.5, diag=_lib.FC_DIAG_WAIT)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.set_localities(loc)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        plain.split_series()
    # an overflowed log is an argument error that names the chain
    small, _ = _make(spec, 2, a0, [0.2, 1.0], 40, pct=0.5)
    small.set_localities(loc)
    small.steps(600)
    ev = small.stats()["events"]
    assert ev[1] > 40
    with pytest.raises(ValueError, match=f"chain {0 if ev[0] > 40 else 1} overflowed event_cap"):
        small.split_series()
    # a ReCom run has no flip log
    a4 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    _, (lo, hi) = G.population_bounds(sec11.n, 4, 0.1)
    cfg = RunConfig(k=4, labels=(0, 1, 2, 3), proposal=_lib.FC_PROPOSE_RECOM, seed=3, pop_lo=lo, pop_hi=hi,
                    diag_mask=0, recom_pop_target=sec11.n / 4, recom_epsilon=0.1)
    recom = FlipRun(FlipGraph(sec11), a4[None, :], cfg)
    with pytest.raises(NotImplementedError):
        recom.set_localities(G.block_localities(sec11, 4, 4))
    with pytest.raises(NotImplementedError):
        recom.split_series()
    # a chain image beyond the LDS limit: 28,900 nodes, each its own locality; one locality fits
    big = G.grid_graph(170, 170)
    plan = G.strip_plan(big, 32)
    wide, _ = _make(big, 32, big.assignment_array(plan, list(range(32))), [1.0], 8, pct=0.5)
    with pytest.raises(NotImplementedError, match="48 KB of LDS"):
        wide.set_localities(np.arange(big.n, dtype=np.int32))
    wide.set_localities(np.zeros(big.n, dtype=np.int32))
    # the largest shape the header promises: n = 16,384 with 256 localities and n_loc k = 4,096
    sq = G.grid_graph(128, 128)
    plan = G.strip_plan(sq, 16)
    fits, _ = _make(sq, 16, sq.assignment_array(plan, list(range(16))), [1.0], 8, pct=0.5)
    fits.set_localities(G.block_localities(sq, 8, 8))
    got = fits.split_series()
    assert got["cells_now"].shape == (1, 256, 16) and int(got["cells_now"].sum()) == sq.n and got["yields"][0] == 1
