"""k = 2 flip kernel: the Philox round keys arrive as the kernel's own second argument.

Every kind of ``flip2_kernel`` instance that reads the key table -- lean, full diagnostics, the
XTRA instance (trace; trace and replay tape), the band stream, and the searching instance
(``FC_FLAG_FORCE_BFS``) -- against the C oracle on a 12 x 12 grid: every statistic the oracle
computes, the final state and, where enabled, every tally, the proposal trace and the event log,
bit for bit, with the 2,000 steps in one launch and in three.  Then the argument's ownership:
two runs with different seeds alive at once and stepped alternately, and a checkpoint restored
into a new run (which fills a key table of its own).
"""
import numpy as np
import pytest

from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from oracle.flipref import STREAM_BAND, STREAM_NODE, draw_tape, events_from_trace

pytestmark = pytest.mark.gpu

STAT_KEYS = ["steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop", "sum_cut", "sum_nb", "sum_wait",
             "sum_cut2", "sum_nb2", "wait_cur", "cut", "nb", "last_flip", "stuck"]
TRACE_FIELDS = ("draw", "v", "flags", "cut", "nb", "wait")
LEAN = _lib.FC_DIAG_WAIT
TALLIES = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST | _lib.FC_DIAG_FLIPS | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_SERIES
SEED, STEPS, CHAINS = 19, 2000, 8
LAUNCHES = [(STEPS,), (667, 667, 666)]

# case -> (diagnostics, trace, tape, band stream, fc_params flags,
#          the instance's FULL / SEARCH / XTRA / BAND template arguments)
CASES = {
    "lean": (0, False, False, False, 0, ("false", "false", "false", "false")),
    "lean_wait": (LEAN, False, False, False, 0, ("false", "false", "false", "false")),
    "full": (TALLIES, False, False, False, 0, ("true", "false", "false", "false")),
    "xtra_trace": (TALLIES, True, False, False, 0, ("true", "false", "true", "false")),
    "xtra_tape_trace": (TALLIES, True, True, False, 0, ("true", "false", "true", "false")),
    "band": (LEAN, False, False, True, 0, ("false", "false", "false", "true")),
    "band_full": (TALLIES, False, False, True, 0, ("true", "false", "false", "true")),
    "force_bfs": (LEAN, False, False, False, _lib.FC_FLAG_FORCE_BFS, ("false", "true", "false", "false")),
    "force_bfs_full": (TALLIES, False, False, False, _lib.FC_FLAG_FORCE_BFS, ("true", "true", "false", "false")),
}

_refs = {}  # oracle runs, computed once and shared between the cases (never modified)


@pytest.fixture(scope="module")
def grid12():
    spec = G.grid_graph(12, 12)
    a0 = spec.assignment_array(G.threshold_plan(spec.nodes, 0, 6), [-1, 1])
    return spec, np.stack([a0] * CHAINS), np.asarray([0.1, 1.0, 10.0] * 3)[:CHAINS]


def _bounds(spec):
    return G.population_bounds(int(spec.pop.sum()), 2, 0.1)[1]


def _ref(cref, grid12, c, band):
    """The oracle's run of chain c (node or band stream) with the trace and every tally."""
    spec, inits, bases = grid12
    if (c, band) not in _refs:
        lo, hi = _bounds(spec)
        _refs[(c, band)] = cref.run(spec, inits[c], base=bases[c], pop_lo=lo, pop_hi=hi, seed=SEED, chain_id=c,
                                    n_steps=STEPS, log1mp=G.log1mp_table(spec.n, 2), trace_cap=400000,
                                    want_hist=True, want_edges=True, want_flips=True,
                                    stream=STREAM_BAND if band else STREAM_NODE)
        assert len(_refs[(c, band)]["trace"]) < 400000
    return _refs[(c, band)]


@pytest.mark.parametrize("launches", LAUNCHES, ids=["one_launch", "three_launches"])
@pytest.mark.parametrize("case", list(CASES))
def test_instances_against_oracle(gpu, cref, grid12, case, launches):
    diag, trace, tape, band, flags, inst = CASES[case]
    spec, inits, bases = grid12
    refs = [_ref(cref, grid12, c, band) for c in range(CHAINS)]
    lo, hi = _bounds(spec)
    cfg = RunConfig(seed=SEED, pop_lo=lo, pop_hi=hi, diag_mask=diag, flags=flags,
                    trace_chains=CHAINS if trace else 0, trace_cap=400000 if trace else 0,
                    event_cap=4096 if diag & _lib.FC_DIAG_SERIES else 0, stream="band" if band else "node")
    run = FlipRun(FlipGraph(spec), inits, cfg, bases=bases)
    if tape:
        # the canonical stream written out (6 words per draw), past the batch window's read-ahead
        n_draws = max(int(r["stats"]["draws"]) for r in refs) + 1024
        run.set_tape(np.stack([draw_tape(SEED, c, n_draws, k=2) for c in range(CHAINS)]))
    for n in launches:
        run.steps(n)
    name = run.kernel_name()
    assert name.startswith("fc::flip2_kernel<8, ") and tuple(x.strip(" >") for x in name.split(",")[2:]) == inst, name
    st, fin = run.stats(), run.state()
    full = bool(diag & _lib.FC_DIAG_HIST)
    if full:
        ch, nh = run.hist()
        ct = run.cut_times()
        nf, ps, lf = run.flips()
    for c, ref in enumerate(refs):
        for k in STAT_KEYS:
            # (diag_mask = 0 draws no geometric waits: the two wait statistics stay 0)
            want = int(ref["stats"][k]) if diag & _lib.FC_DIAG_WAIT or k not in ("sum_wait", "wait_cur") else 0
            assert int(st[k][c]) == want, f"{case} chain {c} stat {k}: {st[k][c]} vs {want}"
        assert np.array_equal(fin[c], ref["final"]), f"{case} chain {c}: final state"
        if full:
            assert np.array_equal(ch[c], ref["cut_hist"]) and np.array_equal(nh[c], ref["nb_hist"]), (case, c)
            assert np.array_equal(ct[c], ref["cut_times"]), (case, c)
            assert np.array_equal(nf[c], ref["num_flips"]) and np.array_equal(ps[c], ref["part_sum"]), (case, c)
            assert np.array_equal(lf[c], ref["last_flipped"]), (case, c)
            ev, exp = run.events(c), events_from_trace(ref["trace"])
            assert len(ev) == len(exp) == st["events"][c], (case, c)
            got = np.stack([ev["t"], ev["v"], ev["cut"], ev["nb"], ev["target"]], axis=1).astype(np.int64)
            assert np.array_equal(got, exp), (case, c)
        if trace:
            tr, rt = run.trace(c), ref["trace"]
            assert len(tr) == len(rt), (case, c, len(tr), len(rt))
            for f in TRACE_FIELDS:
                assert np.array_equal(tr[f], rt[f]), (case, c, f)
    run.close()


def _sec11_setup(sec11, n_chains=4):
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(n_chains)])
    bases = np.asarray([0.1, 1.0, G.SEC11_MU ** 2, 10.0])[:n_chains]
    lo, hi = _bounds(sec11)
    return inits, bases, lo, hi


def _snapshot(run):
    st = run.stats()
    return {k: st[k].copy() for k in STAT_KEYS}, run.state().copy()


def _assert_same(a, b, what):
    for k in STAT_KEYS:
        assert np.array_equal(a[0][k], b[0][k]), (what, k)
    assert np.array_equal(a[1], b[1]), (what, "state")


def test_two_runs_alive_keep_their_own_keys(gpu, sec11):
    """Two runs with different seeds, alive together and stepped alternately (5 x 100 steps, 4
    chains): each ends where the same run does alone -- the launch carries the run's own table."""
    inits, bases, lo, hi = _sec11_setup(sec11)
    fg = FlipGraph(sec11)
    seeds = (101, 0x5EED00020000BEEF)
    alone = []
    for s in seeds:
        r = FlipRun(fg, inits, RunConfig(seed=s, pop_lo=lo, pop_hi=hi), bases=bases)
        for _ in range(5):
            r.steps(100)
        alone.append(_snapshot(r))
        r.close()
    assert not np.array_equal(alone[0][0]["draws"], alone[1][0]["draws"])  # the seeds do differ in effect
    both = [FlipRun(fg, inits, RunConfig(seed=s, pop_lo=lo, pop_hi=hi), bases=bases) for s in seeds]
    for _ in range(5):
        for r in both:
            r.steps(100)
    for i, r in enumerate(both):
        _assert_same(_snapshot(r), alone[i], f"seed {seeds[i]}")
        r.close()


def test_checkpoint_restore_into_new_run(gpu, sec11):
    """500 steps, checkpoint, 500 more; the checkpoint restored into a new run (its own key
    table) and stepped 500 continues bit for bit.  4 chains, lean instance."""
    inits, bases, lo, hi = _sec11_setup(sec11)
    fg = FlipGraph(sec11)
    cfg = RunConfig(seed=77, pop_lo=lo, pop_hi=hi)
    a = FlipRun(fg, inits, cfg, bases=bases)
    a.steps(500)
    blob = a.checkpoint()
    a.steps(500)
    b = FlipRun(fg, inits, cfg, bases=bases)
    b.restore(blob)
    b.steps(500)
    _assert_same(_snapshot(b), _snapshot(a), "restored run")
    a.close()
    b.close()
