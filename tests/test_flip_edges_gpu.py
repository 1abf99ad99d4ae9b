"""GPU parity of the flip kernels with the C oracle at small shapes and on every commit branch.

Every case of ``flip_cases.CASES`` (what each is for, and that the oracle's trace reaches it:
test_flip_cases.py) runs on the device and every chain is compared with ``oracle/flipref.c`` bit
for bit: the per-proposal trace, the counters with ``stuck`` and ``wait_cur``, the final state and
the populations, and with full diagnostics the histograms, ``cut_times`` and the three flip tallies
(what test_parity_gpu.py ``_check_chain`` and test_pair_gpu.py ``_check`` compare; restated here,
since those take one percentage bound for all chains and no draw cap).

The k = 2 cases run under the instances and commit paths a launch can take, because the commit
path is a scheduling choice that must not show: lean and full, the segment-parallel commit for
every acceptance (``par_min`` 1), for none (65) and from three on, windows of 64 and 256 draws,
four chains sharing a workgroup's LDS (the graphs of at most 17 nodes: the smallest chain
footprint), and the band stream.  The k > 2 cases run with the multi-flip commit on and off and
with the forced device search.  Each variant asserts the kernel instance it is meant to select.
"""
import numpy as np
import pytest

import flip_cases as FC
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from oracle.flipref import STREAM_BAND, STREAM_NODE

pytestmark = pytest.mark.gpu

ALL_DIAG = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_FLIPS
LEAN, TALLY, FULL = "lean", "tally", "full"  # waits only | every tally, no trace | every tally and the trace

# k = 2: (diagnostics, tune, band stream).  The instance is <ring, nsub, FULL, SEARCH, XTRA, BAND>:
# FULL with any tally or trace, XTRA with a trace, SEARCH where the graph has nodes the run rule
# does not decide (paths and cycles)
K2_VARIANTS = {
    "full": (FULL, {}, False),
    "full par_min=1 nsub=1": (FULL, {"par_min": 1, "nsub": 1}, False),
    "full par_min=65": (FULL, {"par_min": 65}, False),
    "tally par_min=1": (TALLY, {"par_min": 1}, False),
    "lean": (LEAN, {}, False),
    "lean par_min=1": (LEAN, {"par_min": 1}, False),
    "lean par_min=65 nsub=1": (LEAN, {"par_min": 65, "nsub": 1}, False),
}
SMALL_VARIANTS = {  # n <= 17: four chains in one workgroup's LDS
    "full chains_per_block=4 par_min=1": (FULL, {"chains_per_block": 4, "par_min": 1}, False),
    "lean chains_per_block=4": (LEAN, {"chains_per_block": 4}, False),
}
BAND_VARIANTS = {
    "band full": (FULL, {}, True),
    "band lean par_min=1": (LEAN, {"par_min": 1}, True),
    "band full par_min=65 nsub=1": (FULL, {"par_min": 65, "nsub": 1}, True),
}
K2_PARAMS = [(c.name, v) for c in FC.K2_CASES for v in K2_VARIANTS] + \
            [(c.name, v) for c in FC.K2_CASES if c.spec.n <= 17 for v in SMALL_VARIANTS] + \
            [(c.name, v) for c in FC.K2_CASES if c.band for v in BAND_VARIANTS]
ALL_K2_VARIANTS = {**K2_VARIANTS, **SMALL_VARIANTS, **BAND_VARIANTS}

# k > 2: (diagnostics, tune, flags, needs the district-graph rule)
PAIR_VARIANTS = {
    "multi-flip on": (FULL, {"multi_flip": 1}, 0, False),
    "multi-flip off": (FULL, {"multi_flip": -1}, 0, True),  # without the rule: the same instance as "on"
    "forced search": (FULL, {}, _lib.FC_FLAG_FORCE_BFS, True),  # without the rule: searched anyway
    "lean multi-flip on": (LEAN, {"multi_flip": 1}, 0, False),
}


def _run(case, diag, tune, *, band=False, flags=0):
    nc = case.n_chains
    fg = FlipGraph(case.spec, use_positions=case.use_positions)
    lohi = np.asarray([case.chain_bounds(c) for c in range(nc)], dtype=np.int64)
    traced = diag == FULL
    cfg = RunConfig(k=case.k, labels=case.labels, proposal=_lib.FC_PROPOSE_PAIR if case.pair else _lib.FC_PROPOSE_BI_SIGN,
                    seed=case.seed, pop_lo=int(lohi[0, 0]), pop_hi=int(lohi[0, 1]),
                    diag_mask=_lib.FC_DIAG_WAIT if diag == LEAN else ALL_DIAG, flags=flags,
                    trace_chains=nc if traced else 0, trace_cap=case.trace_cap if traced else 0, tune=dict(tune),
                    stream="band" if band else "node")
    run = FlipRun(fg, np.stack([case.plan(c) for c in range(nc)]), cfg, bases=[case.base(c) for c in range(nc)],
                  pop_bounds=lohi)
    for n in case.launch_steps():  # the device's draw cap is per launch, the oracle's per run
        run.steps(n, max_draws=case.max_draws)
    return fg, run


def _check(case, run, diag, stream=STREAM_NODE):
    """Every chain of the run against the oracle's run of the same chain."""
    st, fin, pops = run.stats(), run.state(), run.pops()
    if diag != LEAN:
        ch, nh = run.hist()
        ct = run.cut_times()
        nf, ps, lf = run.flips()
    for c in range(case.n_chains):
        ref = case.oracle(c, stream)
        who = (case.name, c)
        if diag == FULL:
            tr, rt = run.trace(c), ref["trace"]
            assert len(tr) == len(rt), f"{who}: {len(tr)} vs {len(rt)} proposals"
            for f in FC.TRACE_FIELDS:
                bad = np.nonzero(tr[f] != rt[f])[0]
                assert bad.size == 0, f"{who} field {f} first mismatch at proposal {bad[:1]}: {tr[bad[:3]]} vs {rt[bad[:3]]}"
        for key in FC.STAT_KEYS:
            assert int(st[key][c]) == int(ref["stats"][key]), f"{who} stat {key}: {st[key][c]} vs {ref['stats'][key]}"
        assert np.array_equal(fin[c], ref["final"]), who
        want = np.bincount(ref["final"], weights=case.spec.pop, minlength=case.k).astype(np.int64)
        assert np.array_equal(pops[c], want), who
        if diag != LEAN:
            assert np.array_equal(ch[c], ref["cut_hist"]) and np.array_equal(nh[c], ref["nb_hist"]), who
            assert np.array_equal(ct[c], ref["cut_times"]), who
            assert np.array_equal(nf[c], ref["num_flips"]) and np.array_equal(lf[c], ref["last_flipped"]), who
            assert np.array_equal(ps[c], ref["part_sum"]), who


def _flag(x):
    return "true" if x else "false"


@pytest.mark.parametrize("name,variant", K2_PARAMS)
def test_k2_case_matches_oracle(gpu, name, variant):
    case = FC.BY_NAME[name]
    diag, tune, band = ALL_K2_VARIANTS[variant]
    fg, run = _run(case, diag, tune, band=band)
    search = fg.info["n_exact"] != fg.n
    want = "fc::flip2_kernel<%d, %d, %s, %s, %s, %s>" % (fg.info["ring_max"], tune.get("nsub", 4), _flag(diag != LEAN),
                                                          _flag(search), _flag(diag == FULL), _flag(band))
    assert run.kernel_name() == want
    if tune.get("chains_per_block") == 4:
        # a, fcnt and the two commit marks (npad each), thresholds, search bitmaps, slots, mark sink,
        # wait queue, launch scalars: the footprint fc_run_create documents, at its smallest
        npad, words = (fg.n + 15) // 16 * 16, (fg.n + 63) // 64
        assert (npad, words) in ((16, 1), (32, 1))
        assert run.chain_lds_bytes() == 4 * npad + (2 * 8 + 2) * 8 + 24 * words + 5 * 64 * 4 + 16 + 64 * 24 + 40
    _check(case, run, diag, STREAM_BAND if band else STREAM_NODE)
    run.close()
    fg.close()


@pytest.mark.parametrize("name,variant", [(c.name, v) for c in FC.PAIR_CASES for v, spec in PAIR_VARIANTS.items()
                                          if c.use_positions or not spec[3]])
def test_pair_case_matches_oracle(gpu, name, variant):
    case = FC.BY_NAME[name]
    diag, tune, flags, _ = PAIR_VARIANTS[variant]
    fg, run = _run(case, diag, tune, flags=flags)
    # grids given with positions are planar with exact rings: the district-graph rule (KM = 3)
    # decides every proposal unless the search is forced; without positions the search does (0)
    rule = case.use_positions and not flags
    assert fg.info["n_exact"] == (fg.n if case.use_positions else 0)
    name_ = run.kernel_name()
    assert name_.startswith("fc::flip_kernel<%d, 2, %d, %s, " % (fg.info["ring_max"], 3 if rule else 0,
                                                                  _flag(diag != LEAN))), name_
    multi = rule and tune.get("multi_flip") == 1
    assert name_.endswith((", 1>", ", 2>") if multi else ", 0>"), name_
    if flags or not case.use_positions:
        assert run.stats()["bfs_calls"].sum() > 0
    _check(case, run, diag)
    run.close()
    fg.close()
