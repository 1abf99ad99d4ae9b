"""k = 2 flip kernel: counters and run-length-weighted sums against the C oracle, bit for bit.

The kernel derives ``proposals`` from the steps taken and the two invalid counts, keeps its
counters as partials folded every few batches, and (with the deferred wait queue on) forms
``sum_cut`` / ``sum_nb`` / ``sum_cut2`` / ``sum_nb2`` from the queue entries when the queue is
flushed.  Each case compares every field of ``FlipRun.stats()`` that the oracle computes, and
the final state, with ``cref.run`` (the remaining fields -- search counts, hitting time, event
and series bookkeeping -- have no oracle counterpart and are not touched by these paths).
No trace is requested anywhere here: a trace turns the queue off.
"""
import numpy as np
import pytest

from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

pytestmark = pytest.mark.gpu

STAT_KEYS = ["steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop", "sum_cut", "sum_nb", "sum_wait",
             "sum_cut2", "sum_nb2", "wait_cur", "cut", "nb", "last_flip", "stuck"]
LEAN = _lib.FC_DIAG_WAIT
FULL = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_FLIPS
SEED = 11

_refs = {}  # oracle runs, computed once and shared between the cases (never modified)


def _bounds(spec):
    return G.population_bounds(int(spec.pop.sum()), 2, 0.1)[1]


def _ref(cref, tag, spec, init, base, chain, steps, max_draws=0):
    key = (tag, float(base), chain, steps, max_draws)
    if key not in _refs:
        lo, hi = _bounds(spec)
        _refs[key] = cref.run(spec, init, base=base, pop_lo=lo, pop_hi=hi, seed=SEED, chain_id=chain, n_steps=steps,
                              log1mp=G.log1mp_table(spec.n, 2), max_draws=max_draws)
    return _refs[key]


def _gpu(spec, inits, bases, launches, *, diag, tune=None, max_draws=0):
    lo, hi = _bounds(spec)
    run = FlipRun(FlipGraph(spec), inits, RunConfig(seed=SEED, pop_lo=lo, pop_hi=hi, diag_mask=diag, tune=tune),
                  bases=bases)
    for n in launches:
        run.steps(n, max_draws=max_draws)
    # the instance's third template argument is FULL: the diagnostics choose it
    assert run.kernel_name().split(",")[2].strip() == ("true" if diag != LEAN else "false"), run.kernel_name()
    return run


def _compare(run, refs):
    st, fin = run.stats(), run.state()
    for c, ref in enumerate(refs):
        for k in STAT_KEYS:
            assert int(st[k][c]) == int(ref["stats"][k]), f"chain {c} stat {k}: {st[k][c]} vs {ref['stats'][k]}"
        assert np.array_equal(fin[c], ref["final"]), f"chain {c}: final state"
    run.close()


@pytest.fixture(scope="module")
def grid10():
    spec = G.grid_graph(10, 10)
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 5), [-1, 1])
    return spec, np.stack([a0] * 8), np.asarray([0.1, 1.0, 10.0] * 3)[:8]


def _grid_refs(cref, grid10, steps):
    spec, inits, bases = grid10
    return [_ref(cref, "grid10", spec, inits[c], bases[c], c, steps) for c in range(8)]


@pytest.mark.parametrize("wait_queue", [1, 3, 0])
@pytest.mark.parametrize("launches", [(3000,), (1000, 1000, 1000)])
@pytest.mark.parametrize("diag", [LEAN, FULL], ids=["lean", "full"])
def test_grid10_counters_and_sums(gpu, cref, grid10, diag, launches, wait_queue):
    """10x10 grid, 8 chains at bases 0.1, 1 and 10, 3,000 steps in one launch and in three: the
    counters and the sums across launch boundaries, with the queue flushed at 1, 3 and the
    default number of entries (the start state is unqueued after every flush and at every
    launch's start, queued otherwise)."""
    spec, inits, bases = grid10
    run = _gpu(spec, inits, bases, launches, diag=diag, tune={"wait_queue": wait_queue} if wait_queue else None)
    _compare(run, _grid_refs(cref, grid10, 3000))


@pytest.mark.parametrize("steps", [1, 2, 63])
@pytest.mark.parametrize("diag", [LEAN, FULL], ids=["lean", "full"])
def test_grid10_short_launches(gpu, cref, grid10, diag, steps):
    """Launches of 1, 2 and 63 steps: the last step falls inside a segment or before the first
    acceptance."""
    spec, inits, bases = grid10
    _compare(_gpu(spec, inits, bases, (steps,), diag=diag), _grid_refs(cref, grid10, steps))


@pytest.mark.parametrize("diag", [LEAN, FULL], ids=["lean", "full"])
def test_sec11_stuck_derived_proposals(gpu, cref, sec11, diag):
    """sec11, bases 0.1, 1, 6.96 and 10, 2,000 steps under a draw cap that (by the oracle) ends
    at least one chain stuck before its steps are done: proposals derived from fewer steps than
    the launch asked for."""
    bases = np.asarray([0.1, 1.0, G.SEC11_MU ** 2, 10.0])
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(4)])
    free = [_ref(cref, "sec11s", sec11, inits[c], bases[c], c, 2000) for c in range(4)]
    draws = sorted(int(r["stats"]["draws"]) for r in free)
    cap = (draws[1] + draws[2]) // 2  # between the chains' needs: some finish, some do not
    refs = [_ref(cref, "sec11s", sec11, inits[c], bases[c], c, 2000, cap) for c in range(4)]
    stuck = [c for c in range(4) if int(refs[c]["stats"]["stuck"]) and int(refs[c]["stats"]["steps"]) < 2000]
    assert stuck and len(stuck) < 4, (cap, draws)
    _compare(_gpu(sec11, inits, bases, (2000,), diag=diag, max_draws=cap), refs)


@pytest.mark.parametrize("par_min", [2, 3])
def test_sec11_segment_passes(gpu, cref, sec11, par_min):
    """sec11 at base 1 (nearly every valid proposal accepts), 64 chains, 5,000 steps, segment
    commits from 2 and from 3 acceptances on: passes with many candidates, second mark rounds,
    the foreign-count update."""
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(64)])
    bases = np.ones(64)
    refs = [_ref(cref, "sec11b1", sec11, inits[c], 1.0, c, 5000) for c in range(64)]
    _compare(_gpu(sec11, inits, bases, (5000,), diag=LEAN, tune={"par_min": par_min}), refs)
