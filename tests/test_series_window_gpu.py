"""GPU checks of what the series calls share (DESIGN.md §4 "Series window"): one per-call window
buffer, one output buffer and one indexing convention (per-chain arrays by the call-local chain)
behind ``election_series``, ``shape_series``, ``frame_series``, ``frame_series_changes`` and
``autocorr``.  Every result of a run that interleaves the calls must equal, bit for bit, the same
call made as the only series call of an identically built run.  What each pass computes is checked
against its model in its own file."""
import numpy as np
import pytest

from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

pytestmark = pytest.mark.gpu

BASES = [0.1, 0.38, 1.0, G.SEC11_MU, 10.0, 4.0]
STEPS = 2500
LAGS = [1, 7, 100, 3000]
ELECTIONS = ((2, [(0, 1)], [-200, 0, 200]),  # (columns, elections, gap edges)
             (3, [(0, 2), (2, 1)], [-400, -200, -100, 0, 100, 200, 400]))
PP_EDGES = ([20000, 40000, 50000, 60000], [30000, 55000])


def _votes(n, n_cols):
    return np.random.default_rng(23).integers(0, 2, (n, n_cols)).astype(np.int64)


@pytest.fixture(scope="module")
def build(sec11):
    """build(which) -> a fresh run of 6 chains after 2500 steps, with ELECTIONS[which] and
    PP_EDGES[which] set; every one is the same chain for chain."""
    fg = FlipGraph(sec11)
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(len(BASES))])
    _, (lo, hi) = G.population_bounds(int(sec11.pop.sum()), 2, 0.1)
    cfg = RunConfig(seed=31, pop_lo=lo, pop_hi=hi, diag_mask=_lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES,
                    event_cap=STEPS + 1)

    def settings(run, which):
        n_cols, elections, gap_edges = ELECTIONS[which]
        run.set_elections(_votes(sec11.n, n_cols), elections, gap_edges)
        area, edge_len, ext = G.unit_square_shapes(sec11)
        run.set_shapes(area, edge_len, ext, PP_EDGES[which])

    def make(which=0):
        run = FlipRun(fg, inits, cfg, bases=np.asarray(BASES, dtype=np.float64))
        settings(run, which)
        run.steps(STEPS)
        return run

    make.settings = settings
    return make


def _same(got, want, rows=slice(None)):
    """Every array of `got` equals `want`'s rows `rows`, bit for bit."""
    assert got.keys() == want.keys()
    for key, x in got.items():
        y = want[key][rows]
        assert x.shape == y.shape and x.dtype == y.dtype, key
        assert x.tobytes() == np.ascontiguousarray(y).tobytes(), key


def _same_frames(got, want, rows):
    """frame_series results: the entries below each chain's len (the rest is padding)."""
    assert np.array_equal(got["len"], want["len"][rows])
    for key in ("slope", "angle", "n_cut"):
        for i, c in enumerate(rows):
            m = int(got["len"][i])
            assert got[key][i, :m].tobytes() == want[key][c, :m].tobytes(), (key, c)


def _same_changes(got, want, c0):
    """frame_series_changes of chains c0 .. against the rows of every chain's."""
    nc = got["offsets"].size - 1
    lo, hi = int(want["offsets"][c0]), int(want["offsets"][c0 + nc])
    assert np.array_equal(got["offsets"], want["offsets"][c0:c0 + nc + 1] - lo)
    for key in ("t", "slope", "angle"):
        assert got[key].tobytes() == want[key][lo:hi].tobytes(), key


def test_interleaved_calls_equal_each_call_alone(gpu, sec11, build):
    frame = G.slope_frame(sec11, "sec11")
    run = build()
    got = [run.election_series(2, 3),
           run.shape_series(0, 6),
           run.frame_series_changes(frame, c0=1, nc=4),
           run.autocorr(LAGS),
           run.shape_series(4, 2),
           run.election_series(0, 6),
           run.frame_series(frame, chains=[3, 4])]
    assert got[1]["pp_hist"].sum() == 6 * 2 * (STEPS + 1) and got[5]["seats_hist"].sum() == 6 * (STEPS + 1)
    assert int(got[2]["offsets"][-1]) > 4 and int(got[6]["len"].min()) > 1
    # each call alone on a run of its own
    _same(got[0], build().election_series(2, 3))
    _same(got[1], build().shape_series(0, 6))
    _same_changes(got[2], build().frame_series_changes(frame, c0=1, nc=4), 0)
    for x, y in zip(got[3], build().autocorr(LAGS)):
        assert x.tobytes() == y.tobytes()
    _same(got[4], build().shape_series(4, 2))
    _same(got[5], build().election_series(0, 6))
    _same_frames(got[6], build().frame_series(frame, chains=[3, 4]), [0, 1])
    # a chain range is the rows of every chain's result
    _same(got[0], got[5], slice(2, 5))
    _same(got[4], got[1], slice(4, 6))
    _same_changes(got[2], build().frame_series_changes(frame), 1)
    _same_frames(got[6], build().frame_series(frame), [3, 4])


def test_outputs_resized_by_a_second_setting(gpu, build):
    """Other column, election and edge counts on the same run: the packed outputs are laid out per call."""
    run = build(0)
    run.election_series()
    run.shape_series()
    build.settings(run, 1)
    fresh = build(1)
    _same(run.election_series(), fresh.election_series())
    _same(run.shape_series(1, 4), fresh.shape_series(1, 4))
    assert run.election_series()["tally_now"].shape == (6, 2, 3)
    assert run.shape_series()["pp_hist"].shape == (6, 2, len(PP_EDGES[1]) + 1)


def test_empty_chain_range(gpu, build):
    run = build()
    el = run.election_series(run.n_chains, 0)
    sh = run.shape_series(run.n_chains, 0)
    n_cols, elections, gap_edges = ELECTIONS[0]
    assert el["tally_now"].shape == (0, 2, n_cols) and el["gap_hist"].shape == (0, len(elections), len(gap_edges) + 1)
    assert sh["pp_now"].shape == (0, 2) and sh["pp_min_hist"].shape == (0, len(PP_EDGES[0]) + 1)
    for out in (el, sh):
        assert all(v.size == 0 and v.dtype == np.int64 for v in out.values()) and out["yields"].shape == (0,)
