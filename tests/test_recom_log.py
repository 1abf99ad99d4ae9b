"""ReCom move log, the parts that need no GPU (DESIGN.md "ReCom move log"): the per-yield model
(tests/recom_log_model.py) against the existing event-based models on a flip trajectory; the
``move_cap`` argument checks of ``MarkovChain.run``; and the coverage conditions the GPU cases
(tests/test_recom_log_gpu.py) rely on, asserted on the oracle's trajectories."""
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
from oracle.flipref import events_from_trace

# the GPU cases (tests/test_recom_log_gpu.py) and what each is for
CASES = ("size 2x2 k=2",              # n = 4; accepted steps that move nothing (empty bursts)
         "size 7x9 k=3",              # n = 63: the last compaction pass has 63 lanes
         "size 13x5 k=4",             # n = 65: ... or 1 lane
         "size 16x16 k=4",            # bursts longer than two replay chunks
         "reject 8x8 k=4",            # rejected valid steps (runs longer than one yield)
         "weights 9x7 k=3",           # ... and non-unit populations for pops
         "weights delaunay200 k=3",   # the RMAX = 16 instance
         "k=32 16x16",                # 32 district lanes in the replays
         "many blocks 8x8 k=2")       # 37 chains, four waves per block, chain_id_offset 1000, per-chain bounds


# ---- the model against the event-based models, on a flip trajectory ----------------------------

def _flip_chain(cref, k, steps):
    """The C oracle's flip run on the 8 x 8 grid: (spec, start plan, events, per-yield states)."""
    spec = G.grid_graph(8, 8)
    if k == 2:
        a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 4), [-1, 1])
        kw = dict(labels=[-1, 1])
    else:
        a0 = spec.assignment_array(G.quadrant_plan(spec.nodes, 4), [0, 1, 2, 3])
        kw = dict(labels=[0, 1, 2, 3], proposal=_lib.FC_PROPOSE_PAIR)
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, 0.5)
    r = cref.run(spec, a0, base=1.0, pop_lo=lo, pop_hi=hi, seed=11, chain_id=0, n_steps=steps, k=k,
                 log1mp=G.log1mp_table(spec.n, k), trace_cap=64 * steps, **kw)
    ev = events_from_trace(r["trace"])
    a = np.asarray(a0, dtype=np.int64).copy()
    S, nxt = [], 0
    for t in range(steps + 1):
        while nxt < len(ev) and ev[nxt, 0] <= t:
            a[ev[nxt, 1]] = ev[nxt, 4]
            nxt += 1
        S.append(a.copy())
    assert np.array_equal(S[-1], r["final"])
    return spec, np.asarray(a0, dtype=np.int64), ev, S


@pytest.mark.parametrize("k", [2, 4])
def test_model_agrees_with_event_models_on_flips(cref, k):
    steps = 300
    spec, a0, ev, S_all = _flip_chain(cref, k, steps)
    assert len(ev) > 60
    rng = np.random.default_rng(k)
    cols = rng.integers(0, 50, (spec.n, 3))
    els = [(0, 1), (2, 0)]
    area, edge_len, ext = G.unit_square_shapes(spec)
    loc = G.block_localities(spec, 3, 3)
    pop = np.arange(1, spec.n + 1)
    for t0 in (0, 120):  # the whole run, and a window that starts mid-run
        S = S_all[t0:]
        w = ev[ev[:, 0] > t0]
        cut, nb = M.cut_nb(spec, S)
        # the log, field by field (a flip is a burst of one)
        log, lens = M.expected_log(S, t0, cut, nb)
        assert np.array_equal(log, w[:, [0, 1, 4, 2, 3]]) and lens.max() == 1 and M.straddles(lens) == 0
        # elections
        e0 = EM.replay(S[0], w[:, 0], w[:, 1], w[:, 4], t0, steps, cols, els, [], k)
        edges = EM.spanning_edges(e0["gap_range"])
        want = EM.replay(S[0], w[:, 0], w[:, 1], w[:, 4], t0, steps, cols, els, edges, k)
        got = M.elections(S, cols, els, edges, k)
        assert got["gap_range"] == want["gap_range"]
        for key in EM.KEYS + ("gap_hist", "yields"):
            assert np.array_equal(got[key], want[key]), (t0, key)
        # compactness
        s0 = SM.replay(S[0], w[:, 0], w[:, 1], w[:, 4], t0, steps, spec.edges(), area, ext, edge_len, [], k)
        pp = SM.spanning_edges([s0["q_range"]])
        want = SM.replay(S[0], w[:, 0], w[:, 1], w[:, 4], t0, steps, spec.edges(), area, ext, edge_len, pp, k)
        got = M.shapes(S, spec.edges(), area, ext, edge_len, pp, k)
        assert got["q_range"] == want["q_range"]
        for key in SM.KEYS + ("pp_hist", "pp_min_hist", "yields"):
            assert np.array_equal(got[key], want[key]), (t0, key)
        # locality splits
        want = SPM.replay(S[0], w[:, 0], w[:, 1], w[:, 4], t0, steps, loc, k)
        got = M.splits(S, loc, k)
        for key in SPM.ARRAYS + SPM.SCALARS + ("yields", "x_max"):
            assert np.array_equal(got[key], want[key]), (t0, key)
        # plan samples
        for times in (np.arange(t0, steps + 1), np.arange(t0, steps + 1, 7), np.array([t0, int(w[3, 0]), steps])):
            want = PM.replay(S[0], w, t0, steps, cut[0], nb[0], pop, times, k)
            got = M.plans(S, t0, cut, nb, pop, times, k)
            for key in PM.KEYS:
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (t0, key)
        # lag sums: against numpy on the |cut| series expanded from the events
        x = np.repeat(np.concatenate([[cut[0]], w[:, 2]]), np.diff(np.concatenate([[t0], w[:, 0], [steps + 1]])))
        assert np.array_equal(x, cut)
        lags = [1, 2, 5, len(S) - 1, len(S) + 3]
        assert M.lag_sums(cut, lags).tolist() == [int((x[:len(x) - L] * x[L:]).sum()) if L < len(x) else 0 for L in lags]


def test_model_on_a_burst():
    """Two yields by hand: a step that moves three nodes, then a re-yield."""
    S = [np.array([0, 0, 0, 1, 1, 1]), np.array([0, 1, 1, 1, 0, 1]), np.array([0, 1, 1, 1, 0, 1])]
    log, lens = M.expected_log(S, 10, [1, 3, 3], [2, 5, 5])
    assert log.tolist() == [[11, 1, 1, 3, 5], [11, 2, 1, 3, 5], [11, 4, 0, 3, 5]] and lens.tolist() == [0, 3, 0]
    # log ranges [0, 60), [60, 70) across 64, [70, 71), [71, 128) and [128, 192) up to an edge, [192, 193),
    # [193, 263) across 256
    assert M.straddles(np.array([0, 60, 10, 1, 57, 64, 1, 70])) == 2
    p = M.plans(S, 10, [1, 3, 3], [2, 5, 5], 2 ** np.arange(6), [10, 12], 2)
    assert p["dist0"].tolist() == [0, 3] and p["pops"].tolist() == [[7, 56], [17, 46]] and p["cut"].tolist() == [1, 3]


# ---- MarkovChain.run(move_cap=...) ------------------------------------------------------------

def _partition():
    g = G.sec11_nx()
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "b_nodes": C.b_nodes_bi,
           "base": lambda p: 1.0}
    return C.Partition(g, assignment=G.sec11_plan(0, sorted(g.nodes())), updaters=ups)


def test_move_cap_argument_handling():
    part = _partition()
    pb = C.within_percent_of_ideal_population(part, 0.1)
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.05, node_repeats=1)
    rc = C.MarkovChain(tree, C.Validator([pb]), C.always_accept, part, total_steps=10)
    for bad in (0, -5, 2.5, True, False, "10", "AUTO", ""):  # refused before any device work
        with pytest.raises(ValueError, match="move_cap"):
            rc.run(move_cap=bad)
    with pytest.raises(ValueError, match="sample_every"):  # the other checks still come first
        rc.run(sample_every=0, move_cap="auto")
    with pytest.raises(ValueError, match="move_cap"):  # what a ReCom chain without its log is told
        rc.run(sample_every=5)
    flip = C.MarkovChain(C.slow_reversible_propose_bi, C.Validator([C.single_flip_contiguous, pb]), C.cut_accept, part,
                         total_steps=10)
    for cap in (100, "auto"):
        with pytest.raises(ValueError, match="move_cap"):
            flip.run(move_cap=cap)


# ---- the GPU cases' coverage conditions, on the oracle ----------------------------------------

def _trajectories(name):
    case = RC.BY_NAME[name]
    out = []
    for c in range(case.n_chains):
        S, full = M.states(case, c)
        cut, nb = M.cut_nb(case.spec, S)
        log, lens = M.expected_log(S, 0, cut, nb)
        out.append((S, M.valid_flags(full), log, lens))
    return case, out


@pytest.mark.parametrize("name", CASES)
def test_case_coverage(name):
    case, tr = _trajectories(name)
    assert case.steps == 40 and case.n_chains == (37 if name.startswith("many blocks") else 5)
    for c, (S, flags, log, lens) in enumerate(tr):
        assert len(S) == case.steps + 1 and len(flags) == case.steps
        assert len(log) == lens.sum() <= case.steps * case.spec.n
        # a rejected step re-yields the state
        for t in range(1, len(S)):
            if flags[t - 1] == 1:
                assert lens[t] == 0, (name, c, t)
    if name != "size 2x2 k=2":  # on every other case some chain's burst lies across a chunk boundary
        assert max(M.straddles(lens) for _, _, _, lens in tr) >= 1
    if name == "size 16x16 k=4":
        assert max(int(lens.max()) for _, _, _, lens in tr) > 128
        assert sum(M.straddles(lens) for _, _, _, lens in tr) >= 10
    if name in ("reject 8x8 k=4", "weights 9x7 k=3"):
        for c, (_, flags, _, _) in enumerate(tr):
            assert int((flags == 1).sum()) >= 5, (name, c)
    if name == "size 2x2 k=2":
        assert any(flags[t - 1] == 3 and lens[t] == 0 for _, flags, _, lens in tr for t in range(1, len(lens)))
    if name == "weights delaunay200 k=3":
        assert case.kernel == "fc::recom_kernel<16>"
    if name.startswith("weights"):
        assert len(set(case.spec.pop.tolist())) > 2
