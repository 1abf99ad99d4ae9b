"""GPU checks of the ReCom move log (DESIGN.md "ReCom move log"): a ReCom run created with
FC_DIAG_SERIES and an event_cap logs every accepted step as a burst of events, and every series
pass replays it unchanged.

The reference never goes through events: the state at every yield comes from an oracle run of
that many steps, and tests/recom_log_model.py evaluates every output by its definition at every
yield (tests/test_recom_log.py checks that model against the event-based models on a flip
trajectory, and the coverage conditions of the cases used here).  Everything is compared bit for
bit, for every chain.
"""
import ctypes
import functools

import numpy as np
import pytest

import election_model as EM
import plans_model as PM
import recom_cases as RC
import recom_log_model as M
import shape_model as SM
import split_model as SPM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import EVENT_DTYPE, FlipGraph, FlipRun, RunConfig
from oracle.flipref import recom_run
from test_recom_log import CASES

pytestmark = pytest.mark.gpu

SERIES = _lib.FC_DIAG_SERIES
COUNTERS = ("steps", "proposals", "draws", "accepted", "inv_pop", "sum_cut", "sum_nb", "cut", "nb", "bfs_calls",
            "bfs_levels", "stuck")
ELECTIONS = [(0, 1), (2, 1)]


def _run(case, event_cap, diag=SERIES):
    nc = case.n_chains
    lohi = np.asarray([case.chain_bounds(c) for c in range(nc)], dtype=np.int64)
    cfg = RunConfig(k=case.k, labels=tuple(range(case.k)), proposal=_lib.FC_PROPOSE_RECOM, seed=RC.SEED,
                    pop_lo=int(lohi[0, 0]), pop_hi=int(lohi[0, 1]), base=case.base, chain_id_offset=case.chain_id_offset,
                    recom_pop_target=case.pop_target, recom_epsilon=case.epsilon, recom_node_repeats=case.node_repeats,
                    recom_max_attempts=case.max_attempts, diag_mask=diag, event_cap=event_cap)
    return FlipRun(FlipGraph(case.spec), np.stack([case.plan(c) for c in range(nc)]), cfg,
                   pop_bounds=lohi if len(case.bounds()) > 1 else None)


def _read_events(run, c, cap):
    """The first ``cap`` events of chain c and the number the chain produced (no OverflowError)."""
    out = np.zeros(cap, dtype=EVENT_DTYPE)
    n = ctypes.c_int64(0)
    rc = _lib.load().fc_run_read_events(run.handle, c, ctypes.cast(out.ctypes.data, ctypes.POINTER(_lib.Event)), cap,
                                        ctypes.byref(n))
    assert rc == 0
    return out[:min(cap, n.value)], int(n.value)


def _is_grid(case):
    return all(isinstance(nd, tuple) and len(nd) == 2 for nd in case.spec.nodes) and int(case.spec.degree().max()) <= 4


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Per chain of the case: the per-yield states, |cut|, |B|, the valid steps' flags and the
    expected log; and the case's series inputs.  Computed once, shared, not changed."""
    case = RC.BY_NAME[name]
    spec = case.spec
    chains = []
    for c in range(case.n_chains):
        S, full = M.states(case, c)
        cut, nb = M.cut_nb(spec, S)
        log, lens = M.expected_log(S, 0, cut, nb)
        chains.append(dict(S=S, cut=cut, nb=nb, log=log, lens=lens, flags=M.valid_flags(full), full=full))
    rng = np.random.default_rng(len(name))
    ref = dict(case=case, chains=chains, cols=rng.integers(0, 40, (spec.n, 3)))
    if _is_grid(case):
        ref["shapes"] = G.unit_square_shapes(spec)
        ref["loc"] = G.block_localities(spec, 3, 2)
    return ref


def _assert_log(ev, log):
    assert len(ev) == len(log)
    for j, f in enumerate(("t", "v", "target", "cut", "nb")):
        assert np.array_equal(ev[f].astype(np.int64), log[:, j]), f


def _check_passes(run, ref, t0):
    """Every series pass of ``run`` over its window (yields t0 .. steps) against the model, for
    every chain.  Sets the inputs (the gap / score edges span the model's ranges)."""
    case, cols = ref["case"], ref["cols"]
    spec, k, T = case.spec, case.k, case.steps
    nc = case.n_chains
    W = [dict(S=ch["S"][t0:], cut=ch["cut"][t0:], nb=ch["nb"][t0:], flags=ch["flags"]) for ch in ref["chains"]]
    st = run.stats()
    assert (st["series_t0"] == t0).all() and (st["steps"] == T).all()
    # elections: 3 columns, 2 elections, gap edges across the model's gap range
    ranges = [M.elections(w["S"], cols, ELECTIONS, [], k)["gap_range"] for w in W]
    edges = EM.spanning_edges([(min(r[e][0] for r in ranges), max(r[e][1] for r in ranges)) for e in range(2)])
    run.set_elections(cols, ELECTIONS, edges)
    got = run.election_series()
    for c, w in enumerate(W):
        EM.assert_matches(got, c, M.elections(w["S"], cols, ELECTIONS, edges, k))
    if "shapes" in ref:
        area, edge_len, ext = ref["shapes"]
        qr = [M.shapes(w["S"], spec.edges(), area, ext, edge_len, [], k)["q_range"] for w in W]
        pp = SM.spanning_edges([(min(q[0] for q in qr), max(q[1] for q in qr))])
        run.set_shapes(area, edge_len, ext, pp)
        got = run.shape_series()
        for c, w in enumerate(W):
            SM.assert_matches(got, c, M.shapes(w["S"], spec.edges(), area, ext, edge_len, pp, k))
        run.set_localities(ref["loc"])
        got = run.split_series()
        for c, w in enumerate(W):
            exp = M.splits(w["S"], ref["loc"], k)
            SPM.assert_matches(got, c, exp)
            assert int(got["splits_hist"][c].sum()) == int(got["excess_hist"][c].sum()) == exp["yields"] == T - t0 + 1
    # plan samples: every yield, every 7th, and a list with the window start, a yield made by a
    # rejected step (where the case has one: a re-yield) and the last yield
    rejected = sorted({t for w in W for t in range(t0 + 1, T) if w["flags"][t - 1] == 1})
    mid = rejected[len(rejected) // 2] if rejected else (t0 + T) // 2
    for kw in (dict(every=1), dict(every=7), dict(times=[t0, mid, T])):
        got = run.sample_plans(**kw)
        want_times = np.arange(t0, T + 1, kw["every"]) if "every" in kw else np.asarray(kw["times"])
        assert np.array_equal(got["times"], want_times) and got["plans"].shape == (nc, want_times.size, spec.n)
        for c, w in enumerate(W):
            PM.assert_matches(got, c, M.plans(w["S"], t0, w["cut"], w["nb"], spec.pop, want_times, k))
    # |cut| autocorrelation: the exact lag sums
    lags = [1, 2, 5, T - t0 - 1]
    sums, _ = run.autocorr(lags)
    for c, w in enumerate(W):
        assert np.array_equal(sums[c], M.lag_sums(w["cut"], lags)), (c, sums[c])


@pytest.mark.parametrize("name", CASES)
def test_log_parity(gpu, name):
    """The log of every chain equals the expected log field by field, over two launches; the
    logging instance ran; a twin run without the log ran the lean one to the same states."""
    ref = _reference(name)
    case = ref["case"]
    cap = case.steps * case.spec.n
    run = _run(case, cap)
    run.steps(17).steps(case.steps - 17)
    assert run.kernel_name() == case.kernel.replace("recom_kernel", "recom_log_kernel")
    st, fin = run.stats(), run.state()
    assert (st["events"] <= cap).all()
    for c, ch in enumerate(ref["chains"]):
        _assert_log(run.events(c), ch["log"])
        assert int(st["events"][c]) == len(ch["log"]), (name, c)
        assert np.array_equal(fin[c], ch["S"][-1]), (name, c)
    twin = _run(case, 0, diag=0)
    twin.steps(17).steps(case.steps - 17)
    assert twin.kernel_name() == case.kernel
    st2 = twin.stats()
    assert np.array_equal(twin.state(), fin)
    for key in COUNTERS:
        assert np.array_equal(st[key], st2[key]), (name, key)
    assert (st2["events"] == 0).all()
    run.close()
    twin.close()


@pytest.mark.parametrize("name", CASES)
def test_every_pass_against_the_model(gpu, name):
    ref = _reference(name)
    case = ref["case"]
    run = _run(case, case.steps * case.spec.n)
    run.steps(case.steps)
    _check_passes(run, ref, 0)
    run.close()


def test_window_after_series_reset(gpu):
    """series_reset() after 15 steps, 25 more: the log and every pass over yields 15 .. 40."""
    ref = _reference("size 16x16 k=4")
    case = ref["case"]
    run = _run(case, case.steps * case.spec.n)
    run.steps(15)
    run.series_reset()
    run.steps(case.steps - 15)
    st = run.stats()
    for c, ch in enumerate(ref["chains"]):
        log, _ = M.expected_log(ch["S"][15:], 15, ch["cut"][15:], ch["nb"][15:])
        _assert_log(run.events(c), log)
        assert (int(st["series_cut0"][c]), int(st["series_nb0"][c])) == (ch["cut"][15], ch["nb"][15])
    _check_passes(run, ref, 15)
    run.close()


def test_checkpoint_carries_the_log(gpu):
    """Checkpoint at step 25, restore into a fresh run, finish: the events and the election series
    are byte-identical to the uninterrupted run's."""
    ref = _reference("size 16x16 k=4")
    case, cols = ref["case"], ref["cols"]
    cap = case.steps * case.spec.n
    whole = _run(case, cap)
    whole.steps(case.steps)
    first = _run(case, cap)
    first.steps(25)
    blob = first.checkpoint()
    first.close()
    second = _run(case, cap)
    second.restore(blob)
    second.steps(case.steps - 25)
    edges = np.arange(-400, 401, 50)
    series = []
    for r in (whole, second):
        r.set_elections(cols, ELECTIONS, edges)
        series.append(r.election_series())
    for c, ch in enumerate(ref["chains"]):
        ea, eb = whole.events(c), second.events(c)
        assert ea.tobytes() == eb.tobytes() and len(ea) == len(ch["log"])
    for key in series[0]:
        assert series[0][key].tobytes() == series[1][key].tobytes(), key
    whole.close()
    second.close()


def test_overflow_and_refusals(gpu):
    """A log too small: events counts past the cap, nothing is written past it, every series call
    names a chain; the frame series stays closed to ReCom."""
    case = RC.BY_NAME["size 8x8 k=4"]
    spec = case.spec
    run = _run(case, 40)
    run.steps(case.steps)
    st = run.stats()
    assert (st["events"] > 40).all()
    for c in range(case.n_chains):
        S, _ = M.states(case, c)
        cut, nb = M.cut_nb(spec, S)
        log, _ = M.expected_log(S, 0, cut, nb)
        ev, n_ev = _read_events(run, c, 40)
        assert n_ev == len(log) == int(st["events"][c])
        _assert_log(ev, log[:40])
        assert np.array_equal(run.state()[c], S[-1])
    run.set_elections(np.ones((spec.n, 2), dtype=np.int64), [(0, 1)])
    area, edge_len, ext = G.unit_square_shapes(spec)
    run.set_shapes(area, edge_len, ext)
    run.set_localities(G.block_localities(spec, 4, 4))
    for call in (run.election_series, run.shape_series, run.split_series, lambda: run.sample_plans(every=5),
                 lambda: run.autocorr([1])):
        with pytest.raises(ValueError, match="chain [0-9]+ overflowed"):
            call()
    run.close()
    # frame series: per-event outputs mean nothing inside a burst
    two = RC.BY_NAME["size 2x2 k=2"]
    run = _run(two, two.steps * two.spec.n)
    run.steps(5)
    e = two.spec.edges()
    pos = np.asarray(two.spec.pos, dtype=np.float64)
    frame = G.SlopeFrame(eu=e[:, 0].astype(np.int32), ev=e[:, 1].astype(np.int32),
                         mid=(pos[e[:, 0]] + pos[e[:, 1]]) / 2, center=(0.5, 0.5))
    with pytest.raises(NotImplementedError, match="fc_run_frame_series"):
        run.frame_series(frame)
    # and a ReCom run without the log is told how to get one
    plain = _run(two, 0, diag=0)
    with pytest.raises(NotImplementedError, match="event_cap"):
        plain.sample_plans([0])
    run.close()
    plain.close()


def test_through_the_chain_api(gpu):
    """MarkovChain.run(move_cap="auto") on a partial(recom, ...) chain over sec11, with an Election
    updater and sample_every: plans, elections and rce against per-yield oracle states."""
    g = G.sec11_nx()
    rng = np.random.default_rng(8)
    for nd in g.nodes:
        g.nodes[nd].update(D=int(rng.integers(0, 30)), R=int(rng.integers(0, 30)))
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
           "base": lambda p: 1.0, "E": C.Election("E", {"Dem": "D", "Rep": "R"})}
    part = C.Partition(g, assignment=G.sec11_plan(0, sorted(g.nodes())), updaters=ups)
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.05, node_repeats=1)
    pb = C.within_percent_of_ideal_population(part, 0.1)
    mc = C.MarkovChain(tree, C.Validator([pb]), accept=C.always_accept, initial_state=part, total_steps=21, seed=17,
                       chain_id=2)
    res = mc.run(sample_every=5, move_cap="auto")
    cs = mc.cspec
    S = [np.asarray(cs.init, dtype=np.int64)]
    for t in range(1, 21):
        S.append(np.asarray(recom_run(cs.spec, cs.init, k=2, pop_target=ideal, epsilon=0.05, pop_lo=cs.pop_lo,
                                      pop_hi=cs.pop_hi, seed=17, chain_id=2, n_steps=t)["final"], dtype=np.int64))
    assert res.steps == 20 and res.stats["events"] <= 20 * cs.spec.n
    assert np.array_equal(res.plans["yields"], [0, 5, 10, 15, 20])
    assert np.array_equal(res.plans["assignment"], np.asarray([S[t] for t in (0, 5, 10, 15, 20)], dtype=np.int8))
    cols = np.stack([G.node_columns(g, cs.spec.nodes, ["D", "R"])[c] for c in ("D", "R")], axis=1)
    exp = M.elections(S, cols, [(0, 1)], [], 2)
    r = res.elections["E"]
    assert r["yields"] == 21 and r["gap_sum"] == int(exp["gap_sum"][0])
    assert np.array_equal(r["seats_hist"], exp["seats_hist"][0]) and np.array_equal(r["wins_sum"], exp["wins_sum"][0])
    assert np.array_equal(r["tally_sum"], exp["tally_sum"])
    cut, nb = M.cut_nb(cs.spec, S)
    assert np.array_equal(res.rce, cut) and np.array_equal(res.rbn, nb)
    assert int(res.rce.sum()) == res.rce_sum and int(res.rbn.sum()) == res.rbn_sum
    views = list(res.sampled())
    assert [v.step for v in views] == [0, 5, 10, 15, 20] and len(views[2]["cut_edges"]) == cut[10]
    # without move_cap nothing changes: the updaters are ignored, the counters are the same
    plain = mc.run()
    assert plain.elections is None and plain.plans is None and plain.rce is None
    assert (plain.steps, plain.accepted, plain.rce_sum, plain.final_assignment) == \
        (res.steps, res.accepted, res.rce_sum, res.final_assignment)
