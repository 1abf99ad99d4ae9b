"""GPU checks of the plan samples: ``FlipRun.sample_plans`` -- the device replay of
the accepted-flip log up to chosen yields -- bit for bit against the numpy model
(tests/plans_model.py) fed with the same run's ``events()``, window-start states and ``stats()``;
two checks that do not go through the log (a twin run read launch by launch, and the per-step
iterator); and the call's edges and errors.  ``event_cap`` >= steps + 1 everywhere but the
overflow case, so no chain is left out."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import plans_model as PM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from test_splits_gpu import _grid_3000, _grid_run, _kgt2_case, _make

pytestmark = pytest.mark.gpu

I64 = ctypes.POINTER(ctypes.c_int64)
I8 = ctypes.POINTER(ctypes.c_int8)


def _check(run, starts, times, c0=0, nc=None, **kw):
    """Sample chains [c0, c0 + nc) at ``times`` and compare each with the model.  Returns the
    device's result and the models."""
    nc = run.n_chains - c0 if nc is None else nc
    times = np.asarray(times, dtype=np.int64)
    got = run.sample_plans(times, c0=c0, nc=nc, **kw)
    assert np.array_equal(got["times"], times)
    st = run.stats()
    assert np.array_equal(got["yields"], (st["steps"] - st["series_t0"] + 1)[c0:c0 + nc])
    models = []
    for i in range(nc):
        m = PM.replay_run(run, c0 + i, starts[c0 + i], times)
        PM.assert_matches(got, i, m)
        models.append(m)
    return got, models


def _check_now(run, got, j, c0=0):
    """Sample ``j`` (taken at the chains' last yield) is ``state()`` and ``pops()``."""
    nc = got["cut"].shape[0]
    st = run.stats()
    assert np.array_equal(got["plans"][:, j], run.state()[c0:c0 + nc])
    assert np.array_equal(got["pops"][:, j], run.pops()[c0:c0 + nc])
    assert np.array_equal(got["cut"][:, j], st["cut"][c0:c0 + nc]) and np.array_equal(got["nb"][:, j], st["nb"][c0:c0 + nc])


def test_grid_k2_every_pattern(gpu):
    """n = 132 (rows have padding), six bases, 3000 steps.  The model's counters are those of the
    CPU oracle for exactly these inputs (chain ids 0-5): no chain passes without several events on
    one node inside one chunk of 64 and inside one interval between two samples."""
    spec, run, inits = _grid_3000()
    st = run.stats()
    assert st["events"].tolist() == [1757, 3000, 2287, 1768, 1346, 1113] and (st["steps"] == 3000).all()
    got, ms = _check(run, inits, np.arange(0, 3001, 7))
    assert all(m["chunk_same_node"] > 0 and m["repeat_between"] > 0 for m in ms)
    assert sum(m["chunk_same_node"] for m in ms) >= 5166 and sum(m["repeat_between"] for m in ms) >= 676
    assert all(len(set(m["dist0"].tolist())) >= 30 for m in ms)
    assert (got["pops"].sum(axis=2) == spec.n).all() and (got["dist0"][:, 0] == 0).all()
    # every yield: several samples per chunk, samples between events, on an event's t and on t - 1
    got, _ = _check(run, inits, np.arange(0, 3001))
    _check_now(run, got, 3000)
    assert np.array_equal(got["plans"][:, 0], inits) and (got["dist0"][:, 0] == 0).all()
    assert np.array_equal(got["cut"][:, 0], st["series_cut0"]) and np.array_equal(got["nb"][:, 0], st["series_nb0"])
    kernel_ms, copy_ms = run.sample_plans_ms()  # device time of that call's kernel and row copy
    assert kernel_ms > 0 and copy_ms > 0
    run.sample_plans([0, 3000], plans=False)
    assert run.sample_plans_ms()[0] > 0 and run.sample_plans_ms()[1] == 0
    # whole chunks applied between two samples
    _check(run, inits, np.arange(0, 3001, 500))
    got, _ = _check(run, inits, [0])
    assert np.array_equal(got["plans"][:, 0], inits)
    got, _ = _check(run, inits, [3000])
    _check_now(run, got, 0)
    # times all before a chain's first event, and all after its last
    before = after = 0
    for c in range(run.n_chains):
        ev = run.events(c)
        first, last = int(ev["t"][0]), int(ev["t"][-1])
        got, _ = _check(run, inits, np.arange(0, first), c0=c, nc=1)
        assert (got["dist0"] == 0).all() and (got["plans"] == inits[c]).all()
        before += first > 1
        if last < 3000:
            got, _ = _check(run, inits, np.arange(last + 1, 3001), c0=c, nc=1)
            assert (got["plans"] == run.state()[c]).all()
            after += 1
        _check(run, inits, np.arange(last, 3001), c0=c, nc=1)
    assert after > 0


def test_twin_run_read_launch_by_launch(gpu):
    """Independent of the log: a twin run stepped 500 at a time, ``state()`` read after each
    launch, holds the samples of the one-launch run at 500, 1000, ..., 3000.  And a run of three
    launches of 1000 steps gives the outputs of the one launch of 3000."""
    _, run, inits = _grid_3000()
    times = np.arange(500, 3001, 500)
    got = run.sample_plans(times)
    _, twin, _ = _grid_run(3000)
    for j in range(times.size):
        twin.steps(500)
        st = twin.stats()
        assert np.array_equal(twin.state(), got["plans"][:, j]) and np.array_equal(twin.pops(), got["pops"][:, j])
        assert np.array_equal(st["cut"], got["cut"][:, j]) and np.array_equal(st["nb"], got["nb"][:, j])
    _, three, _ = _grid_run(3000)
    for _ in range(3):
        three.steps(1000)
    x, y = run.sample_plans(every=7), three.sample_plans(every=7)
    assert x["times"].size == 429
    for key in x:
        assert np.array_equal(x[key], y[key]), key


def test_through_the_chain_api(gpu, tmp_path):
    """``MarkovChain.run(sample_every=50)`` holds the assignments, |cut| and |B| the per-step
    iterator yields at ``i % 50 == 0``; ``sampled()`` and ``save_plans`` round-trip."""
    g = nx.grid_graph([10, 10])
    for nd in g.nodes:
        g.nodes[nd]["population"] = 1 + (nd[0] + 2 * nd[1]) % 3
    plan = {nd: (1 if nd[0] >= 5 else -1) for nd in g.nodes}
    updaters = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
                "base": lambda p: 1.3}
    part = C.Partition(g, plan, updaters)
    popbound = C.within_percent_of_ideal_population(part, 0.3)

    def chain():
        return C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, popbound]),
                             accept=C.cut_accept, initial_state=part, total_steps=1001, seed=9)
    mc = chain()
    res = mc.run(series=False, corrected=False, sample_every=50)
    assert res.rce is None and set(res.plans) == {"yields", "assignment", "cut", "nb", "dist0", "pops"}
    assert res.plans["yields"].tolist() == list(range(0, 1001, 50)) and res.plans["assignment"].shape == (21, 100)
    nodes, labels = mc.cspec.spec.nodes, mc.cspec.labels
    seen = 0
    for i, st in enumerate(chain()):
        if i % 50:
            continue
        j = i // 50
        assert [st.assignment[nd] for nd in nodes] == [labels[d] for d in res.plans["assignment"][j]], i
        assert len(st["cut_edges"]) == res.plans["cut"][j] and len(st["b_nodes"]) == res.plans["nb"][j]
        assert [st["population"][lab] for lab in labels] == res.plans["pops"][j].tolist()
        seen += 1
    assert seen == 21 and res.plans["dist0"][0] == 0 and res.plans["dist0"].max() > 0
    assert res.final_assignment == {nd: labels[d] for nd, d in zip(nodes, res.plans["assignment"][-1])}
    views = list(res.sampled())
    assert [v.step for v in views] == res.plans["yields"].tolist()
    for j, v in enumerate(views):
        assert len(v["cut_edges"]) == res.plans["cut"][j] and len(v["b_nodes"]) == res.plans["nb"][j]
        assert [v["population"][lab] for lab in labels] == res.plans["pops"][j].tolist()
        assert sorted(len(p) for p in v.parts.values()) == sorted(np.bincount(res.plans["assignment"][j]).tolist())
        assert v["base"] == 1.3 and v.flips is None
        with pytest.raises(KeyError):
            v["geom"]
    path = res.save_plans(str(tmp_path / "plans"))
    assert path.endswith("plans.npz")
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["nodes", "labels"] + list(res.plans))
        assert z["nodes"].tolist() == [list(nd) for nd in nodes] and z["labels"].tolist() == labels
        for key, val in res.plans.items():
            assert np.array_equal(z[key], val) and z[key].dtype == val.dtype, key
    # the default changes nothing
    plain = chain().run(series=False, corrected=False)
    assert plain.plans is None and plain.final_assignment == res.final_assignment
    assert (plain.steps, plain.proposals, plain.accepted) == (res.steps, res.proposals, res.accepted)


def test_chunk_boundaries_windows_and_ranges(gpu):
    """The base-1 chain read at 0, 64 and 65 logged events; a window reset at yield 1000 read at
    absolute times; chain sub-ranges; nc = 0 and n_times = 0; every output NULL in turn."""
    spec, run, inits = _grid_run(200, bases=[1.0])
    _check(run, inits, [0])
    for want in (64, 65):
        for _ in range(200):  # one step per launch: the count grows by at most one
            if int(run.stats()["events"][0]) == want:
                break
            run.steps(1)
        assert int(run.stats()["events"][0]) == want
        T = int(run.stats()["steps"][0])
        got, _ = _check(run, inits, np.arange(0, T + 1))
        _check_now(run, got, T)
    spec, run, inits = _grid_run(3000)
    run.steps(1000)
    run.series_reset()
    starts = run.state()
    got, _ = _check(run, starts, [1000])
    assert (got["dist0"] == 0).all()
    run.steps(2000)
    st = run.stats()
    assert (st["series_t0"] == 1000).all() and (st["events"] > 64).all()
    got, _ = _check(run, starts, np.arange(1000, 3001))
    _check_now(run, got, 2000)
    assert np.array_equal(run.sample_plans(every=400)["times"], [1000, 1400, 1800, 2200, 2600, 3000])
    with pytest.raises(ValueError, match="chain 0: time 999 is before"):
        run.sample_plans([999, 1000])
    whole, _ = _check(run, starts, np.arange(1000, 3001, 7))
    part, _ = _check(run, starts, np.arange(1000, 3001, 7), c0=2, nc=3)
    for key in PM.KEYS:
        assert np.array_equal(part[key], whole[key][2:5]), key
    _check(run, starts, np.arange(1003, 2990, 13), c0=5, nc=1)
    empty = run.sample_plans([1000, 2000], c0=3, nc=0)
    assert empty["plans"].shape == (0, 2, spec.n) and empty["pops"].shape == (0, 2, 2) and empty["yields"].shape == (0,)
    none = run.sample_plans(np.zeros(0, dtype=np.int64))
    assert none["plans"].shape == (6, 0, spec.n) and none["cut"].shape == (6, 0)
    # any output may be NULL; what is left is written as before
    L = _lib.load()
    times = np.arange(1000, 3001, 7, dtype=np.int64)
    m = times.size
    full = {"plans": whole["plans"], "cut": whole["cut"], "nb": whole["nb"], "dist0": whole["dist0"], "pops": whole["pops"]}
    for skip in list(full) + ["all", "none"]:
        bufs = {key: np.full_like(val, -3) for key, val in full.items()}
        ptrs = [None if skip in (key, "all") else bufs[key].ctypes.data_as(I8 if key == "plans" else I64) for key in full]
        assert L.fc_run_sample_plans(run.handle, 0, 6, m, times.ctypes.data_as(I64), *ptrs) == _lib.FC_OK, skip
        for key in full:
            if skip in (key, "all"):
                assert (bufs[key] == -3).all(), (skip, key)
            else:
                assert np.array_equal(bufs[key], full[key]), (skip, key)
    assert "plans" not in run.sample_plans(times, plans=False) and "pops" not in run.sample_plans(times, pops=False)
    # nc = 0 and n_times = 0 write nothing, whatever the pointers
    buf = np.full(4, -3, dtype=np.int64)
    assert L.fc_run_sample_plans(run.handle, 2, 0, m, times.ctypes.data_as(I64), None, buf.ctypes.data_as(I64), None,
                                 None, None) == _lib.FC_OK
    assert L.fc_run_sample_plans(run.handle, 0, 6, 0, None, None, buf.ctypes.data_as(I64), None, None, None) == _lib.FC_OK
    assert (buf == -3).all()


def test_grid_quadrants_k4(gpu):
    """12 x 12 grid, quadrant plan, PAIR proposals: targets 0 .. 3, per-node population adds."""
    spec = G.grid_graph(12, 12)
    a0 = spec.assignment_array(G.quadrant_plan(spec.nodes, 6), [0, 1, 2, 3])
    run, inits = _make(spec, 4, a0, [0.3, 1.0, 2.0], 2501, pct=0.5)
    run.steps(2500)
    assert int(run.stats()["events"].min()) > 64
    got, ms = _check(run, inits, np.arange(0, 2501))
    _check_now(run, got, 2500)
    got, ms = _check(run, inits, np.arange(0, 2501, 7))
    assert all(m["chunk_same_node"] > 0 and m["repeat_between"] > 0 for m in ms)
    assert (got["pops"].sum(axis=2) == spec.n).all() and got["plans"].max() == 3
    _check(run, inits, [5, 1250, 2500], c0=1, nc=2)


@pytest.mark.parametrize("name", ["triangular_k8", "delaunay_k18", "delaunay_k32"])
def test_kgt2(gpu, name):
    """k > 2 up to every district in use, so targets reach 31."""
    spec, k, a0 = _kgt2_case(name)
    steps = 1500
    run, inits = _make(spec, k, a0, [0.5, 2.0], steps + 1, pct=0.1, tune={"multi_flip": 1})
    run.steps(steps)
    assert int(run.stats()["events"].min()) > 64
    got, ms = _check(run, inits, np.arange(0, steps + 1, 7))
    assert got["plans"].max() == k - 1 and all(m["dist0"].max() > 0 for m in ms)
    got, _ = _check(run, inits, np.arange(steps - 40, steps + 1), c0=1, nc=1)
    _check_now(run, got, 40, c0=1)


def test_sec11_k2(gpu, sec11):
    """sec11 at k = 2: 16 chains, 20,000 steps, stride 1000."""
    a0 = sec11.assignment_array(G.sec11_plan(0, sec11.nodes), [-1, 1])
    bases = [0.4, 0.8, 1.0, 1.25] * 4
    run, inits = _make(sec11, 2, a0, bases, 20001, pct=0.1, seed=5)
    run.steps(20000)
    assert int(run.stats()["events"].min()) > 64
    got, ms = _check(run, inits, np.arange(0, 20001, 1000))
    _check_now(run, got, 20)
    assert all(m["repeat_between"] > 0 for m in ms) and got["dist0"][:, -1].min() > 0
    assert len({got["plans"][c, -1].tobytes() for c in range(16)}) == 16  # the chains differ


def test_n_16384(gpu):
    """The 128 x 128 grid: 1024 vectors of 16 nodes per row, 2 chains, 500 steps, 11 samples."""
    spec = G.grid_graph(128, 128)
    a0 = spec.assignment_array(G.strip_plan(spec, 2), [0, 1])
    run, inits = _make(spec, 2, a0, [0.8, 1.0], 501, pct=0.5)
    run.steps(500)
    assert int(run.stats()["events"].min()) > 64
    got, ms = _check(run, inits, np.arange(0, 501, 50))
    _check_now(run, got, 10)
    assert all(m["dist0"].max() > 0 for m in ms)


def test_interleaving_checkpoint_and_restore(gpu):
    """Calls between the other series passes leave their results alone and read the same; a blob
    taken after a call equals, byte for byte, the one taken before; a run restored from it is
    sampled at once and reads what the uninterrupted run reads."""
    spec, run, inits = _grid_run(1500)
    cols = np.random.default_rng(23).integers(0, 2, (spec.n, 2))
    run.set_elections(cols, [(0, 1)], [-20, 0, 20])
    run.set_shapes(*G.unit_square_shapes(spec), [100, 1000, 10000])
    run.set_localities(G.block_localities(spec, 2, 3))
    e = spec.edges()
    on_rim = np.array([spec.nodes[u][0] == spec.nodes[v][0] == 0 or spec.nodes[u][1] == spec.nodes[v][1] == 0
                       for u, v in e])
    xy = np.asarray(spec.nodes, dtype=np.float64)
    frame = G.SlopeFrame(eu=e[on_rim, 0].astype(np.int32), ev=e[on_rim, 1].astype(np.int32),
                         mid=(xy[e[on_rim, 0]] + xy[e[on_rim, 1]]) / 2, center=(5.5, 5.0))
    assert frame.eu.size == 21
    run.steps(800)
    times = np.arange(0, 801, 7)

    def others():
        return [run.election_series(), run.shape_series(), run.split_series(), run.frame_series(frame)]
    before = others()
    blob_before = run.checkpoint()
    first, _ = _check(run, inits, times)
    assert run.checkpoint() == blob_before
    mid = others()
    second, _ = _check(run, inits, times, c0=1, nc=4)
    after = others()
    for x, y, z in zip(before, mid, after):
        for key in x:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes() == np.asarray(z[key]).tobytes(), key
    for key in PM.KEYS:
        assert np.array_equal(second[key], first[key][1:5]), key
    _, back, _ = _grid_run(1500)
    back.restore(blob_before)
    restored = back.sample_plans(times)  # no setter: a restored run is sampled at once
    for key in first:
        assert np.array_equal(restored[key], first[key]), key
    for r in (run, back):
        r.steps(700)
    x, y = run.sample_plans(every=11), back.sample_plans(every=11)
    for key in x:
        assert np.array_equal(x[key], y[key]), key
    _check(back, inits, np.arange(0, 1501, 11))


def test_error_codes(gpu, sec11):
    spec, run, inits = _grid_run(500)
    run.steps(500)
    L = _lib.load()
    with pytest.raises(ValueError, match="no fc_run_sample_plans call recorded"):
        run.sample_plans_ms()
    t = np.array([0, 100, 500], dtype=np.int64)
    tp = t.ctypes.data_as(I64)

    def raw(c0, nc, n_times, times):
        rc = L.fc_run_sample_plans(run.handle, c0, nc, n_times, times, None, None, None, None, None)
        return rc, (L.fc_last_error() or b"").decode()
    assert raw(0, 6, 3, tp)[0] == _lib.FC_OK
    for c0, nc in ((-1, 2), (0, 7), (6, 1), (2, -1)):
        rc, msg = raw(c0, nc, 3, tp)
        assert rc == _lib.FC_ERR_ARG and "fc_run_sample_plans: chain range" in msg
        with pytest.raises(ValueError, match="chain range"):
            run.sample_plans(t, c0=c0, nc=nc)
    rc, msg = raw(0, 6, -1, tp)
    assert rc == _lib.FC_ERR_ARG and "fc_run_sample_plans: n_times" in msg
    rc, msg = raw(0, 6, 3, None)
    assert rc == _lib.FC_ERR_ARG and "fc_run_sample_plans: null times" in msg
    for bad in ([0, 100, 100], [0, 200, 100]):
        b = np.array(bad, dtype=np.int64)
        rc, msg = raw(0, 6, 3, b.ctypes.data_as(I64))
        assert rc == _lib.FC_ERR_ARG and "fc_run_sample_plans: times must be strictly increasing" in msg
    with pytest.raises(ValueError, match="chain 0: time 501 is after"):
        run.sample_plans([0, 501])
    with pytest.raises(ValueError, match="chain 2: time -1 is before"):
        run.sample_plans([-1, 5], c0=2, nc=2)
    assert L.fc_run_sample_plans(None, 0, 1, 0, None, None, None, None, None, None) == _lib.FC_ERR_ARG
    # no FC_DIAG_SERIES
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    plain, _ = _make(spec, 2, a0, [1.0], 0, pct=0.5, diag=_lib.FC_DIAG_WAIT)
    with pytest.raises(ValueError, match="fc_run_sample_plans: FC_DIAG_SERIES"):
        plain.sample_plans([0])
    # an overflowed log is an argument error that names the chain
    small, _ = _make(spec, 2, a0, [0.2, 1.0], 40, pct=0.5)
    small.steps(600)
    ev = small.stats()["events"]
    assert ev[1] > 40
    with pytest.raises(ValueError, match=f"fc_run_sample_plans: chain {0 if ev[0] > 40 else 1} overflowed event_cap"):
        small.sample_plans([0, 600])
    # a ReCom run has no flip log
    a4 = sec11.assignment_array(G.quadrant_plan(sec11.nodes), [0, 1, 2, 3])
    _, (lo, hi) = G.population_bounds(sec11.n, 4, 0.1)
    cfg = RunConfig(k=4, labels=(0, 1, 2, 3), proposal=_lib.FC_PROPOSE_RECOM, seed=3, pop_lo=lo, pop_hi=hi,
                    diag_mask=0, recom_pop_target=sec11.n / 4, recom_epsilon=0.1)
    recom = FlipRun(FlipGraph(sec11), a4[None, :], cfg)
    with pytest.raises(NotImplementedError, match="fc_run_sample_plans"):
        recom.sample_plans([0])
