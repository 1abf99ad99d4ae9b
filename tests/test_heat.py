"""Heat-map series, the parts that need no GPU: the per-yield model
(tests/heat_model.py) against the C oracle's fused tallies on flip trajectories and by hand on a
burst; the coverage conditions the GPU cases (tests/test_heat_gpu.py) rely on, asserted on the
oracle's trajectories; and the neighbour / edge rows the replay walks, slot by slot."""
import functools

import numpy as np
import pytest

import heat_model as HM
import recom_cases as RC
import recom_log_model as M
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph
from oracle.flipref import events_from_trace
from test_recom_log import CASES, _trajectories

K4_LABELS = (3, -2, 7, 0)  # as tests/test_corrected_stats_gpu.py
SEED = 23


@functools.lru_cache(maxsize=None)
def flip_setup(name):
    """The flip runs of the heat-map tests, CPU and GPU: graph, start plan, labels, proposal, bases."""
    if name == "grid8 k=2":
        spec = G.grid_graph(8, 8)
        a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 4), [-1, 1])
        return dict(name=name, spec=spec, k=2, a0=a0, labels=(-1, 1), proposal=_lib.FC_PROPOSE_BI_SIGN, pct=0.5,
                    bases=(1.0, 0.4, 2.5))
    side = {"grid8 k=4": 8, "grid12 k=4": 12}[name]
    spec = G.grid_graph(side, side)
    a0 = spec.assignment_array(G.quadrant_plan(spec.nodes, side // 2), [0, 1, 2, 3])
    return dict(name=name, spec=spec, k=4, a0=a0, labels=K4_LABELS, proposal=_lib.FC_PROPOSE_PAIR, pct=0.5,
                bases=(1.0, 0.3, 2.0))


_FLIPS = {}  # (setup name, chain, steps) -> (per-yield states, oracle run): computed once, shared, not changed


def flip_states(cref, name, c, steps):
    """Chain c of a flip setup on the C oracle: the state at every yield 0 .. steps (rebuilt from the
    trace's accepted flips, as test_recom_log._flip_chain does) and the oracle's run with its fused
    tallies."""
    key = (name, c, steps)
    if key not in _FLIPS:
        fs = flip_setup(name)
        spec, k = fs["spec"], fs["k"]
        _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, fs["pct"])
        r = cref.run(spec, fs["a0"], base=fs["bases"][c], pop_lo=lo, pop_hi=hi, seed=SEED, chain_id=c, n_steps=steps,
                     k=k, labels=list(fs["labels"]), proposal=fs["proposal"], log1mp=G.log1mp_table(spec.n, k),
                     trace_cap=64 * steps + 4096, want_hist=True, want_edges=True, want_exact_flips=True)
        ev = events_from_trace(r["trace"])
        a = np.asarray(fs["a0"], dtype=np.int64).copy()
        S, nxt = [], 0
        for t in range(steps + 1):
            while nxt < len(ev) and ev[nxt, 0] <= t:
                a[ev[nxt, 1]] = ev[nxt, 4]
                nxt += 1
            S.append(a.copy())
            S[-1].setflags(write=False)
        assert nxt == len(ev) and np.array_equal(S[-1], r["final"])
        _FLIPS[key] = (S, r)
    return _FLIPS[key]


def model_of(spec, S, t0, k):
    cut, nb = M.cut_nb(spec, S)
    return HM.heat(S, t0, spec.edges(), k, cut, nb, G.nb_width(spec, k, False))


# ---- the model against the C oracle's fused tallies --------------------------------------------

@pytest.mark.parametrize("name", ["grid8 k=2", "grid8 k=4"])
def test_model_agrees_with_the_oracle(cref, name):
    fs = flip_setup(name)
    S, ref = flip_states(cref, name, 0, 300)
    assert int(ref["stats"]["accepted"]) > 60
    m = model_of(fs["spec"], S, 0, fs["k"])
    assert m["yields"] == 301
    assert np.array_equal(m["cut_hist"], ref["cut_hist"]) and np.array_equal(m["nb_hist"], ref["nb_hist"])
    assert np.array_equal(m["cut_times"], ref["cut_times"])
    assert np.array_equal(m["moves"], ref["flip_count"]) and np.array_equal(m["last_move"], ref["last_accept"])
    assert np.array_equal(HM.occupancy(m["dwell"], fs["labels"]), ref["occupancy"])
    assert (m["dwell"].sum(axis=1) == 301).all() and m["cut_hist"].sum() == m["nb_hist"].sum() == 301


def test_model_on_a_burst():
    """A path of six nodes by hand: one step moves three nodes, two of them adjacent, then a
    re-yield.  Yields 10, 11, 12."""
    uv = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    S = [np.array([0, 0, 0, 1, 1, 1]), np.array([0, 0, 1, 0, 1, 0]), np.array([0, 0, 1, 0, 1, 0])]
    m = HM.heat(S, 10, uv, 2, [1, 4, 4], [2, 5, 5], 7)
    assert m["yields"] == 3
    assert m["cut_hist"].tolist() == [0, 1, 0, 0, 2, 0] and m["nb_hist"].tolist() == [0, 0, 1, 0, 0, 2, 0]
    # (2, 3) is cut before and after the step that moves both its ends
    assert m["cut_times"].tolist() == [0, 2, 3, 2, 2]
    assert m["moves"].tolist() == [0, 0, 1, 1, 0, 1] and m["last_move"].tolist() == [0, 0, 11, 11, 0, 11]
    assert m["dwell"].tolist() == [[3, 0], [3, 0], [1, 2], [2, 1], [0, 3], [2, 1]]
    assert HM.occupancy(m["dwell"], (-1, 1)).tolist() == [-3, -3, 1, -1, 3, -1]
    assert HM.moved_edge_ends(S, uv) == 1 and HM.flipped_back(S) == 0
    assert HM.flipped_back([np.array([0, 1]), np.array([1, 1]), np.array([1, 1]), np.array([0, 1])]) == 1


# ---- the GPU cases' coverage conditions, on the oracle ----------------------------------------

def test_recom_case_coverage():
    """Among the ReCom cases the GPU test runs: an accepted step that moves nothing, a burst that
    moves both ends of an edge, a burst across a multiple of 64 in the log index, and a run longer
    than one yield."""
    empty = both_ends = straddle = reyield = 0
    for name in CASES:
        case, tr = _trajectories(name)
        uv = case.spec.edges()
        for S, flags, log, lens in tr:
            empty += sum(1 for t in range(1, len(lens)) if flags[t - 1] == 3 and lens[t] == 0)
            both_ends += HM.moved_edge_ends(S, uv)
            straddle += M.straddles(lens)
            reyield += int((lens[1:] == 0).sum())
    assert empty >= 1 and both_ends >= 1 and straddle >= 1 and reyield >= 1


@pytest.mark.parametrize("name", ["grid8 k=2", "grid12 k=4"])
def test_flip_case_coverage(cref, name):
    """The flip runs contain a node that is flipped and flipped back."""
    S, ref = flip_states(cref, name, 0, 2000)
    assert HM.flipped_back(S) >= 1 and int(ref["flip_count"].max()) >= 2


def test_dwell_on_a_recom_chain_needs_the_log():
    """Refused before any device work, like sample_every."""
    from flipcomplexityempirical_amd import chain as C
    from test_recom_log import _partition
    part = _partition()
    pb = C.within_percent_of_ideal_population(part, 0.1)
    ideal = sum(part["population"].values()) / len(part)
    tree = functools.partial(C.recom, pop_col="population", pop_target=ideal, epsilon=0.05, node_repeats=1)
    rc = C.MarkovChain(tree, C.Validator([pb]), C.always_accept, part, total_steps=10)
    with pytest.raises(ValueError, match="move_cap"):
        rc.run(dwell=True)


# ---- the neighbour / edge rows ----------------------------------------------------------------

@pytest.mark.parametrize("graph", ["grid", "triangular", "delaunay200"])
def test_neighbour_rows(graph):
    spec = {"grid": lambda: G.grid_graph(7, 9), "triangular": lambda: G.triangular_graph(6, 7),
            "delaunay200": RC.delaunay200}[graph]()
    uv = spec.edges()
    nbr, eid = FlipGraph(spec).heat_rows()
    deg = spec.degree()
    W = nbr.shape[1]
    assert nbr.shape == eid.shape == (spec.n, W) and W == (8 if int(deg.max()) <= 8 else 16)
    if graph == "delaunay200":
        assert W == 16
    seen = np.zeros(len(uv), dtype=np.int64)
    for u in range(spec.n):
        d = int(deg[u])
        assert (nbr[u, d:] == -1).all() and (eid[u, d:] == -1).all()
        for j in range(d):  # every slot's edge joins u and the slot's neighbour
            e = int(eid[u, j])
            assert 0 <= e < len(uv) and sorted((u, int(nbr[u, j]))) == sorted(uv[e].tolist()), (u, j)
            seen[e] += 1
        assert len(set(eid[u, :d].tolist())) == d
    assert (seen == 2).all()  # every canonical edge in the rows of both its ends, once each
