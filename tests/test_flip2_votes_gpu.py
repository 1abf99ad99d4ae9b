"""flip2_kernel's wave votes, held as lane masks, against the C oracle at the shapes where a mask can go wrong.

The k = 2 kernel holds every predicate of a batch's commit as a 64-bit lane mask: one vote per
compare, the conjunctions, negations, inequalities and lane ranges composed with scalar operations
(fc_device.h ``vote`` / ``lanes``).  A mask differs from the vote over the composed bool where a
lane that holds no slot, a lane outside the commit's range [pos, end) or a lane past the launch's
last step leaks into it, so the cases here put such lanes beside live ones:

* graphs of fewer than 64 nodes (3 x 3, 4 x 4, the 9 x 7 grid with populations 1-59): a batch
  rarely fills its 64 slots, so idle lanes sit beside live ones in every vote;
* launches of 1, 2 and 3 steps, and launches that end inside a window in which a later proposal is
  accepted: with ``par_min`` 1 the launch's last step lies inside a segment pass (``last_step``);
* an 8 x 8 grid whose windows of 256 draws hold 63, 64 and more than 64 boundary hits: the batch
  that just fits its slots, and the one the 64th hit closes;
* population bounds that bind, so that a slot's verdict under the acceptances before it differs
  from its speculative one (``cand1 != cand0``) and closes the segment;
* ``par_min`` 1 (every acceptance takes the segment pass) and 65 (none does: one event at a time),
  the default in between; the node stream and the band stream; lean, tally and full diagnostics.

Every chain is compared with ``oracle/flipref.c`` bit for bit, on what
``test_flip_edges_gpu._check`` compares.  The CPU tests state from the oracle's trace alone that
each case reaches what it is for.
"""
import functools

import numpy as np
import pytest

import flip_cases as FC
from oracle.flipref import FLAG_ACCEPTED, FLAG_VALID, STREAM_BAND, STREAM_NODE
from recom_cases import both_strips, grid
from test_flip_edges_gpu import FULL, LEAN, TALLY, _check, _flag, _run

SHORT = (1, 2, 3, 5, 40)  # steps of the first launches


def _case(name, graph, bounds, ok, **kw):
    kw.setdefault("bases", (1.0, 0.5, 3.0))
    return FC.Case(name, graph, 2, both_strips, bounds, ok, steps=1500, launches=SHORT, n_chains=8, band=True, **kw)


CASES = [
    _case("votes grid3x3", functools.partial(grid, 3, 3), FC.pct_bounds(0.5), FC.both_invalid_kinds),
    _case("votes grid4x4", functools.partial(grid, 4, 4), FC.pct_bounds(0.5), FC.all_steps),
    # bounds about two median nodes wide: verdicts change under the acceptances before them
    _case("votes grid9x7 weighted", FC.small_weights_grid, FC.around_start(40), FC.verdict_flips(5),
          bases=(1.0, 0.7, 1.5)),
    # a quarter of the nodes on the boundary: a window of 256 draws holds about 64 hits
    _case("votes grid8x8", functools.partial(grid, 8, 8), FC.pct_bounds(0.5), FC.all_steps),
]
for _c in CASES:  # the oracle cache of flip_cases looks its cases up by name
    assert FC.BY_NAME.setdefault(_c.name, _c) is _c
SMALL = [c.name for c in CASES[:3]]

VARIANTS = {  # (diagnostics, tune, band stream)
    "lean": (LEAN, {}, False),
    "lean par_min=1": (LEAN, {"par_min": 1}, False),
    "lean par_min=65": (LEAN, {"par_min": 65}, False),
    "lean par_min=1 nsub=1": (LEAN, {"par_min": 1, "nsub": 1}, False),
    "tally par_min=65": (TALLY, {"par_min": 65}, False),
    "full par_min=1": (FULL, {"par_min": 1}, False),
    "band lean par_min=1": (LEAN, {"par_min": 1}, True),
    "band full par_min=65": (FULL, {"par_min": 65}, True),
}


# ---- CPU: the oracle's trace reaches what each case is for ---------------------------------------
def _launch_ends(case, trace):
    """Per launch but the last: (first proposal of the launch, proposal of its last step)."""
    valid = np.nonzero((trace["flags"] & FLAG_VALID) != 0)[0]
    out, start, done = [], 0, 0
    for n in case.launch_steps()[:-1]:
        done += n
        last = int(valid[done - 1])  # every valid proposal is one step
        out.append((start, last))
        start = last + 1  # the next launch starts at the draw after its last step's
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_reaches_the_case(case):
    assert case.launch_steps()[:3] == [1, 2, 3]
    for stream in (STREAM_NODE, STREAM_BAND):
        inside = 0
        for c in range(case.n_chains):
            ref = case.oracle(c, stream)
            assert case.chain_ok(case, c, ref), (case.name, c, stream)
            tr = ref["trace"]
            assert len(tr) < case.trace_cap
            acc = (tr["flags"] & FLAG_ACCEPTED) != 0
            for start, last in _launch_ends(case, tr):
                # the launch's last step and a later acceptance in the launch's first 64 proposals:
                # with par_min = 1 the commit of that batch is a segment pass, and the step ends inside it
                inside += int(last - start < FC.WINDOW and acc[last + 1:start + FC.WINDOW].any())
        assert inside >= case.n_chains, (case.name, stream, inside)


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs_leave_lanes_idle(name):
    case = FC.BY_NAME[name]
    assert case.spec.n < FC.WINDOW
    # proposals are draws on boundary nodes: fewer than one per draw leaves slots of a 64-draw window empty
    for c in range(case.n_chains):
        s = case.oracle(c)["stats"]
        assert s["proposals"] < s["draws"], (name, c)


def _window_hits(trace, width=256):
    """Proposals in the draw window of a batch that starts right after each proposal's draw."""
    d = trace["draw"].astype(np.int64)
    lo = d + 1
    hi = lo + width - (lo & 3)  # the node stream's window ends with the last lane's Philox call
    return np.searchsorted(d, hi, side="left") - np.searchsorted(d, lo, side="left")


def test_windows_hold_63_64_and_more_hits():
    case = FC.BY_NAME["votes grid8x8"]
    hits = np.concatenate([_window_hits(case.oracle(c)["trace"]) for c in range(case.n_chains)])
    for want in (63, 64):
        assert (hits == want).sum() >= 5, (want, np.bincount(hits)[56:72])
    assert (hits > 64).sum() >= 20 and (hits < 63).sum() >= 20


def test_population_bounds_close_segments():
    case = FC.BY_NAME["votes grid9x7 weighted"]
    for c in range(case.n_chains):
        ref = case.oracle(c)
        lo, hi = case.chain_bounds(c)
        assert FC.pop_verdict_flips(case.spec.pop, 2, case.plan(c), ref["trace"], lo, hi) >= 5, c
        assert ref["stats"]["inv_pop"] > 0, c  # the bounds bind: proposals are refused by population


# ---- GPU -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [(c.name, v) for c in CASES for v in VARIANTS])
def test_case_matches_oracle(gpu, name, variant):
    case = FC.BY_NAME[name]
    diag, tune, band = VARIANTS[variant]
    fg, run = _run(case, diag, tune, band=band)
    want = "fc::flip2_kernel<8, %d, %s, false, %s, %s>" % (tune.get("nsub", 4), _flag(diag != LEAN), _flag(diag == FULL),
                                                          _flag(band))
    assert run.kernel_name() == want
    _check(case, run, diag, STREAM_BAND if band else STREAM_NODE)
    run.close()
    fg.close()
