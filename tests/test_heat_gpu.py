"""GPU checks of the heat-map series: ``FlipRun.heat_series`` -- the device replay of
the event log into the |cut| / |B| histograms, per-edge cut times, per-node moves, last moves and
district dwell times -- bit for bit, every chain, every array.

Two references that share nothing with the replay: for ReCom runs the per-yield model
(tests/heat_model.py) on oracle states, one oracle run per yield (tests/recom_log_model.py); for
flip runs the same run's fused tallies (``hist()``, ``cut_times()``, ``flips_exact()``), kept by the
flip kernels as they step.  tests/test_heat.py checks the model and the cases' coverage conditions
on the CPU."""
import ctypes
import functools

import numpy as np
import pytest

import heat_model as HM
import recom_cases as RC
import recom_log_model as M
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from oracle.flipref import recom_run
from test_heat import SEED, flip_setup, flip_states, model_of
from test_recom_log import CASES
from test_recom_log_gpu import _reference, _run

pytestmark = pytest.mark.gpu

I64 = ctypes.POINTER(ctypes.c_int64)
FUSED = _lib.FC_DIAG_SERIES | _lib.FC_DIAG_HIST | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_FLIPS_EXACT


def _same(a, b):
    """Two heat_series results, byte for byte."""
    assert set(a) == set(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def _invariants(got):
    y = got["yields"]
    assert (got["cut_hist"].sum(axis=1) == y).all() and (got["nb_hist"].sum(axis=1) == y).all()
    assert (got["dwell"].sum(axis=2) == y[:, None]).all()
    assert (got["cut_times"] >= 0).all() and (got["cut_times"] <= y[:, None]).all()
    assert ((got["last_move"] == 0) == (got["moves"] == 0)).all()


# ---- 1, 2: ReCom runs against the model, in both forms ------------------------------------------

@functools.lru_cache(maxsize=None)
def _logged(name):
    """The case's logged ReCom run after all its steps, and the model of every chain's window."""
    ref = _reference(name)
    case = ref["case"]
    run = _run(case, case.steps * case.spec.n)
    run.steps(case.steps)
    uv = case.spec.edges()
    models = [HM.heat(ch["S"], 0, uv, case.k, ch["cut"], ch["nb"], run.nb_width()) for ch in ref["chains"]]
    return case, run, models


@pytest.mark.parametrize("name", CASES)
def test_recom_against_the_model(gpu, name):
    case, run, models = _logged(name)
    got = run.heat_series()
    assert run.heat_series_info()["form"] == "global_rows" and run.heat_series_info()["ms"] > 0
    assert got["dwell"].shape == (case.n_chains, case.spec.n, case.k)
    for c, m in enumerate(models):
        HM.assert_matches(got, c, m)
    _invariants(got)
    if name.startswith("many blocks"):
        for c0, nc in ((0, 37), (5, 9), (36, 1)):
            part = run.heat_series(c0, nc)
            for i in range(nc):
                HM.assert_matches(part, i, models[c0 + i])


@pytest.mark.parametrize("name", CASES)
def test_recom_both_forms(gpu, name):
    case, run, models = _logged(name)
    lds = run.heat_series(lds_rows=True)
    info = run.heat_series_info()
    assert info["form"] == "lds"
    rows = run.heat_series()
    info_g = run.heat_series_info()
    assert info_g["form"] == "global_rows" and info_g["lds_bytes"] < info["lds_bytes"]
    _same(lds, rows)
    for c, m in enumerate(models):
        HM.assert_matches(rows, c, m)
    # a subset of the outputs: the arrays move up in the LDS image
    some = run.heat_series(want=("nb_hist", "dwell"), lds_rows=True)
    assert set(some) == {"nb_hist", "dwell", "yields"}
    assert some["nb_hist"].tobytes() == lds["nb_hist"].tobytes() and some["dwell"].tobytes() == lds["dwell"].tobytes()


# ---- 3: flip runs against the fused tallies ---------------------------------------------------

def _flip_run(name, cap, diag=FUSED, bases=None):
    fs = flip_setup(name)
    spec, k = fs["spec"], fs["k"]
    bases = fs["bases"] if bases is None else bases
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, fs["pct"])
    cfg = RunConfig(k=k, labels=tuple(fs["labels"]), proposal=fs["proposal"], seed=SEED, pop_lo=lo, pop_hi=hi,
                    diag_mask=diag, event_cap=cap)
    return FlipRun(FlipGraph(spec), np.stack([fs["a0"]] * len(bases)), cfg, bases=np.asarray(bases, dtype=np.float64))


def _check_fused(run, labels, form="global_rows", **kw):
    """The window from yield 0 against the run's own fused tallies."""
    got = run.heat_series(**kw)
    assert run.heat_series_info()["form"] == form
    assert (run.stats()["series_t0"] == 0).all()
    ch, nh = run.hist()
    xf, xo, xl = run.flips_exact()
    assert np.array_equal(got["cut_hist"], ch) and np.array_equal(got["nb_hist"], nh)
    assert np.array_equal(got["cut_times"], run.cut_times())
    assert np.array_equal(got["moves"], xf) and np.array_equal(got["last_move"], xl)
    assert np.array_equal(got["dwell"] @ np.asarray(labels, dtype=np.int64), xo)
    assert np.array_equal(got["yields"], run.stats()["steps"] + 1)
    _invariants(got)
    return got


@functools.lru_cache(maxsize=None)
def _flips_2000(name):
    run = _flip_run(name, 2001)
    run.steps(700).steps(600).steps(700)
    return run


@pytest.mark.parametrize("name", ["grid8 k=2", "grid12 k=4"])
def test_flips_against_the_fused_tallies(gpu, name):
    run = _flips_2000(name)
    st = run.stats()
    assert (st["steps"] == 2000).all() and int(st["events"].min()) > 128
    got = _check_fused(run, flip_setup(name)["labels"])
    assert int(got["moves"].max()) >= 2
    _same(got, _check_fused(run, flip_setup(name)["labels"], form="lds", lds_rows=True))


def test_sec11_mixed_bases_against_the_fused_tallies(gpu, sec11):
    n_chains, steps = 16, 5000
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(n_chains)])
    bases = np.asarray([G.SEC11_BASES[c % 10] for c in range(n_chains)])
    _, (lo, hi) = G.population_bounds(sec11.n, 2, 0.1)
    cfg = RunConfig(seed=31, pop_lo=lo, pop_hi=hi, diag_mask=FUSED, event_cap=steps + 1)
    run = FlipRun(FlipGraph(sec11), inits, cfg, bases=bases)
    run.steps(steps)
    _same(_check_fused(run, (-1, 1)), _check_fused(run, (-1, 1), form="lds", lds_rows=True))
    run.close()


# ---- 4: windows and chunk edges ---------------------------------------------------------------

def test_chunk_edges_and_windows(gpu, cref):
    name = "grid8 k=2"
    fs = flip_setup(name)
    spec = fs["spec"]
    run = _flip_run(name, 1501, diag=FUSED | _lib.FC_DIAG_WAIT)  # (the oracle draws the waits too)
    for want in (0, 1, 63, 64, 65, 127, 128, 129):  # (from 128 on the second chunk read ahead is refilled)
        for _ in range(200):  # one step per launch: the count grows by at most one
            if int(run.stats()["events"][0]) == want:
                break
            run.steps(1)
        assert int(run.stats()["events"][0]) == want
        got = _check_fused(run, fs["labels"])
        _same(got, _check_fused(run, fs["labels"], form="lds", lds_rows=True))
        T = int(run.stats()["steps"][0])
        for c in range(run.n_chains):
            HM.assert_matches(got, c, model_of(spec, flip_states(cref, name, c, 1500)[0][:T + 1], 0, 2))
    # a window that starts mid-run: yields 700 .. 1500 against the model on oracle states
    run.steps(700 - int(run.stats()["steps"][0]))
    run.series_reset()
    one = run.heat_series()  # a window of the single yield 700
    state, st = run.state(), run.stats()
    uv = spec.edges()
    for c in range(run.n_chains):
        assert one["yields"][c] == 1 and (one["moves"][c] == 0).all() and (one["last_move"][c] == 0).all()
        assert np.array_equal(one["cut_hist"][c], np.bincount([st["cut"][c]], minlength=len(uv) + 1))
        assert np.array_equal(one["nb_hist"][c], np.bincount([st["nb"][c]], minlength=run.nb_width()))
        assert np.array_equal(one["cut_times"][c], (state[c][uv[:, 0]] != state[c][uv[:, 1]]).astype(np.int64))
        assert np.array_equal(one["dwell"][c], np.eye(2, dtype=np.int64)[state[c]])
    run.steps(800)
    assert (run.stats()["series_t0"] == 700).all() and int(run.stats()["events"].min()) > 64
    got = run.heat_series()
    for c in range(run.n_chains):
        S = flip_states(cref, name, c, 1500)[0]
        assert np.array_equal(S[-1], run.state()[c])
        HM.assert_matches(got, c, model_of(spec, S[700:], 700, 2))
    _same(got, run.heat_series(lds_rows=True))
    run.close()


# ---- 5: a chain that does not fit LDS ---------------------------------------------------------

def test_large_graph_takes_global_rows(gpu):
    spec = G.grid_graph(128, 128)
    a0 = spec.assignment_array(G.strip_plan(spec, 2), [0, 1])
    _, (lo, hi) = G.population_bounds(spec.n, 2, 0.5)
    cfg = RunConfig(seed=SEED, pop_lo=lo, pop_hi=hi, diag_mask=FUSED, event_cap=3001)
    run = FlipRun(FlipGraph(spec), np.stack([a0, a0]), cfg, bases=np.asarray([1.0, 0.5]))
    run.steps(3000)
    assert int(run.stats()["events"].min()) > 64
    _check_fused(run, (-1, 1), form="global_rows", lds_rows=True)  # asked for, but the image does not fit
    assert run.heat_series_info()["lds_bytes"] < 160 * 1024
    run.close()


# ---- 6: through the chain API -----------------------------------------------------------------

def test_through_the_chain_api(gpu):
    g = G.sec11_nx()
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
           "base": lambda p: 1.0}
    part = C.Partition(g, assignment=G.sec11_plan(0, sorted(g.nodes())), updaters=ups)
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.05, node_repeats=1)
    pb = C.within_percent_of_ideal_population(part, 0.1)
    mc = C.MarkovChain(tree, C.Validator([pb]), accept=C.always_accept, initial_state=part, total_steps=21, seed=17,
                       chain_id=2)
    res = mc.run(move_cap="auto")
    cs = mc.cspec
    spec = cs.spec
    S = [np.asarray(cs.init, dtype=np.int64)]
    for t in range(1, 21):
        S.append(np.asarray(recom_run(spec, cs.init, k=2, pop_target=ideal, epsilon=0.05, pop_lo=cs.pop_lo,
                                      pop_hi=cs.pop_hi, seed=17, chain_id=2, n_steps=t)["final"], dtype=np.int64))
    m = model_of(spec, S, 0, 2)
    assert res.steps == 20 and int(m["moves"].sum()) == res.stats["events"] > 0
    assert np.array_equal(res.cut_hist, m["cut_hist"]) and np.array_equal(res.nb_hist, m["nb_hist"])
    assert list(res.cut_times) == [(spec.nodes[u], spec.nodes[v]) for u, v in spec.edges()]
    assert list(res.cut_times.values()) == m["cut_times"].tolist()
    assert [res.flip_count[nd] for nd in spec.nodes] == m["moves"].tolist()
    assert [res.last_accept[nd] for nd in spec.nodes] == m["last_move"].tolist()
    assert [res.occupancy[nd] for nd in spec.nodes] == HM.occupancy(m["dwell"], cs.labels).tolist()
    assert res.dwell.dtype == np.int64 and np.array_equal(res.dwell, m["dwell"])
    assert res.num_flips == {} and res.part_sum == {} and res.last_flipped == {}
    # without move_cap a ReCom chain returns the empty fields it always did
    plain = mc.run()
    assert plain.cut_hist.size == 0 and plain.nb_hist.size == 0 and plain.cut_times == {} and plain.num_flips == {}
    assert plain.flip_count is None and plain.occupancy is None and plain.last_accept is None and plain.dwell is None
    assert (plain.steps, plain.accepted, plain.final_assignment) == (res.steps, res.accepted, res.final_assignment)


def test_flip_chain_dwell_keyword(gpu):
    """A flip chain fills ``dwell`` only when asked, and it integrates to the corrected occupancy."""
    g = G.sec11_nx()
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
           "base": lambda p: 1.3}
    part = C.Partition(g, assignment=G.sec11_plan(0, sorted(g.nodes())), updaters=ups)
    pb = C.within_percent_of_ideal_population(part, 0.1)
    mc = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, pb]), accept=C.cut_accept,
                       initial_state=part, total_steps=501, seed=9)
    res = mc.run(series=False, dwell=True)
    nodes = mc.cspec.spec.nodes
    assert res.dwell.shape == (len(nodes), 2) and (res.dwell.sum(axis=1) == 501).all()
    lab = mc.cspec.dev_labels if mc.cspec.dev_labels is not None else range(2)
    assert [res.occupancy[nd] for nd in nodes] == HM.occupancy(res.dwell, list(lab)).tolist()
    assert mc.run(series=False).dwell is None and mc.run().dwell is None


# ---- 7: refusals ------------------------------------------------------------------------------

def test_refusals(gpu):
    L = _lib.load()
    run = _flip_run("grid8 k=2", 0, diag=_lib.FC_DIAG_HIST)
    with pytest.raises(ValueError, match="FC_DIAG_SERIES"):
        run.heat_series()
    run.close()
    run = _flip_run("grid8 k=2", 10, bases=(1.0, 1.0))
    run.steps(5)
    for c0, nc in ((0, 3), (2, 1), (-1, 1), (0, -1)):
        with pytest.raises(ValueError, match="chain range"):
            run.heat_series(c0, nc)
    buf = np.full(65, -3, dtype=np.int64)
    assert L.fc_run_heat_series(run.handle, 0, 1, 0x2, None, None, None, buf.ctypes.data_as(I64), None, None) == \
        _lib.FC_ERR_ARG and b"unknown flags" in L.fc_last_error()
    # nc = 0 and no output asked for are FC_OK and write nothing
    assert L.fc_run_heat_series(run.handle, 1, 0, 0, None, None, None, buf.ctypes.data_as(I64), None, None) == _lib.FC_OK
    assert L.fc_run_heat_series(run.handle, 0, 2, 0, None, None, None, None, None, None) == _lib.FC_OK
    assert (buf == -3).all()
    with pytest.raises(ValueError, match="unknown outputs"):
        run.heat_series(want=("cut_hist", "waits"))
    run.steps(200)
    assert (run.stats()["events"] > 10).all()
    with pytest.raises(ValueError, match="chain [0-9]+ overflowed"):
        run.heat_series()
    run.close()
    two = RC.BY_NAME["size 2x2 k=2"]
    plain = _run(two, 0, diag=0)
    with pytest.raises(NotImplementedError, match="event_cap"):
        plain.heat_series()
    plain.close()


# ---- 8: interleaving --------------------------------------------------------------------------

def test_interleaving_and_checkpoint(gpu):
    run = _flips_2000("grid8 k=2")
    spec = flip_setup("grid8 k=2")["spec"]
    blob = run.checkpoint()
    cols = np.random.default_rng(5).integers(0, 40, (spec.n, 2))
    run.set_elections(cols, [(0, 1)])
    e1 = run.election_series(0, 2)
    h1 = run.heat_series(1, 2)
    p1 = run.sample_plans(every=100, c0=0, nc=3)
    h0 = run.heat_series(0, 1, lds_rows=True)
    e2 = run.election_series(0, 2)
    h2 = run.heat_series(1, 2)
    p2 = run.sample_plans(every=100, c0=0, nc=3)
    whole = run.heat_series()
    for a, b in ((e1, e2), (p1, p2)):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    _same(h1, h2)
    for key in whole:
        assert np.array_equal(whole[key][1:3], h1[key]) and np.array_equal(whole[key][0:1], h0[key]), key
    assert run.checkpoint() == blob
