"""The k = 2 tally case table shared by test_tally_cases.py (CPU: every case's oracle run and pass
plan reach what the case is for) and test_tally_edges_gpu.py (the device's histograms, cut_times,
quirk and corrected flip tallies equal the oracle's on every chain of every case and variant).

What is under test is the tally path of the k = 2 full-diagnostics instance: flip2_kernel's
tally_flush, the 16-byte log entry of csrc/fc_tally.h, and tally_reduce_kernel with the pass plan
of csrc/fc_tally_plan.h.  Every case is k = 2 on the node stream, BI_SIGN, untraced; a case is a
``flip_cases.Case`` (graph, plans, bounds, bases, seed, steps, launches) plus the variants it runs
under: (diagnostics, flags, tune) each.  The groups:

``plan``      the five grids of the hand-written plan table (tests/native/tally_plan_check.cpp)
              and sec11, the one-pass control: 1,500 steps as launches of 700, 1 and 799, so a
              plan is launched three times and ``tl_len`` is cleared between them
``ring16``    a Delaunay graph whose rings need the 16-cell record and whose cut histogram and
              cut_times are above the LDS limit: tally_reduce_kernel<16>, edges by global atomics
``subset``    (variants of the 48 x 48 grid) each tally diagnostic alone and two pairs, which
              leave holes in the kernel's LDS offsets
``overflow``  FC_FLAG_TALLY_LOG_SMALL (a 64-entry log) against the full log, queue lengths 1, 5, 64
``long``      runs of 256 and of 65,536 yields and more: the two carries of tally_pack's run field
``edge``      one call of 2^23 steps (dt uses bit 22) and one of 2^23 + 5 (two launches)

The oracle runs here ask for the corrected tallies as well (``want_exact_flips``), and the long
cases for no 16,384-record trace, so this table keeps its own oracle cache; its names are kept
apart from ``flip_cases.BY_NAME`` (test_flip_cases.py runs every name of that table through
conditions written for graphs of at most 65 nodes, so these cases are not entered there).
"""
import dataclasses
import functools
import os
import shutil
import subprocess
from typing import Sequence

import numpy as np

import flip_cases as FC
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from oracle.flipref import events_from_trace
from recom_cases import both_strips, grid, strips

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")

WAIT, HIST, EDGES, FLIPS, EXACT = (_lib.FC_DIAG_WAIT, _lib.FC_DIAG_HIST, _lib.FC_DIAG_EDGES, _lib.FC_DIAG_FLIPS,
                                   _lib.FC_DIAG_FLIPS_EXACT)
ALL = WAIT | HIST | EDGES | FLIPS | EXACT
SMALL = _lib.FC_FLAG_TALLY_LOG_SMALL
LIMIT = 163840  # gfx950's dynamic LDS per workgroup: the limit the hand table is written for
# array bits of a pass plan, in tally_reduce_kernel's order
CUT, NB, EDGE, NF, PS, LF, FCN, OCC, LA = (1 << a for a in range(9))


# ---- graphs and plans ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def delaunay7000():
    return G.delaunay_graph(7000, seed=0)


@functools.lru_cache(maxsize=None)
def delaunay_wide():
    """test_flip2_neighbours_gpu.py's graph of 60 points whose longest ring needs the 16-cell record."""
    return G.delaunay_graph(60, seed=3)


def middle(spec, k):
    """A straight cut down the middle of a lattice of (x, y) nodes."""
    xs = sorted(set(nd[0] for nd in spec.nodes))
    return [spec.assignment_array(G.threshold_plan(spec.nodes, 0, (xs[0] + xs[-1] + 1) / 2), [-1, 1])]


# ---- coverage conditions: (case, chain, oracle result) -> bool ------------------------------------
def all_steps(case, c, ref):
    s = ref["stats"]
    return s["steps"] == case.steps and s["stuck"] == 0 and s["accepted"] > 0


def run_lengths(case, ref):
    """Yields of every state of the run, from the accepted flips' yields alone."""
    t = ref["events"][:, 0]
    return np.diff(np.concatenate([[0], t, [case.steps + 1]]))


def long_runs(case, c, ref):
    """At least 10 runs whose length carries into tally_pack's second word only (256 .. 65,535
    yields) and 5 that use its upper byte there (65,536 and more)."""
    r = run_lengths(case, ref)
    return all_steps(case, c, ref) and int(((r >= 256) & (r < 65536)).sum()) >= 10 and int((r >= 65536).sum()) >= 5


def late_flips(case, c, ref):
    """Accepted flips in the launch's second half (dt >= 2^22: bit 22) and, where the call is
    longer than one launch of 2^23 steps, in the launch after it."""
    last = int(ref["last_accept"].max())
    return all_steps(case, c, ref) and last >= 1 << 22 and (case.steps <= 1 << 23 or last > 1 << 23)


@dataclasses.dataclass(frozen=True)
class TallyCase(FC.Case):
    group: str = ""
    variants: Sequence = ()     # (label, diagnostics, flags, tune)
    want_events: bool = False   # the oracle keeps the accepted flips (t, v, cut, nb, target)
    slow: bool = False          # the device test is marked slow

    def oracle(self, c):
        return _oracle(self.name, c)


@functools.lru_cache(maxsize=None)
def _oracle(name, c):
    case = BY_NAME[name]
    spec = case.spec
    lo, hi = case.chain_bounds(c)
    cap = case.steps + (1 << 20) if case.want_events else 0
    ref = FC._cref().run(spec, case.plan(c), base=case.base(c), pop_lo=lo, pop_hi=hi, seed=case.seed, chain_id=c,
                         n_steps=case.steps, k=2, labels=list(case.labels), log1mp=G.log1mp_table(spec.n, 2),
                         max_draws=0, trace_cap=cap, want_hist=True, want_edges=True, want_flips=True,
                         want_exact_flips=True)
    if case.want_events:
        trace = ref.pop("trace")
        assert len(trace) == ref["stats"]["proposals"] < cap
        ref["events"] = events_from_trace(trace)
    for arr in ref.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return ref


def _case(name, graph, group, variants, **kw):
    kw.setdefault("plans", middle)
    kw.setdefault("bounds", FC.pct_bounds(0.5))
    kw.setdefault("chain_ok", all_steps)
    kw.setdefault("bases", (0.5, 1.0, 2.0, G.SEC11_MU))
    kw.setdefault("n_chains", 4)
    return TallyCase(name=name, graph=graph, k=2, max_draws=0, trace_cap=0, group=group, variants=tuple(variants), **kw)


EVERY = ("all", ALL, 0, {})
SUBSETS = [("HIST", WAIT | HIST, 0, {}), ("EDGES", WAIT | EDGES, 0, {}), ("FLIPS", WAIT | FLIPS, 0, {}),
           ("FLIPS_EXACT", WAIT | EXACT, 0, {}),
           ("HIST+FLIPS_EXACT", WAIT | HIST | EXACT, 0, {}),  # arrays 0, 1, 6-8: a hole of four in off[]
           ("EDGES+FLIPS_EXACT", WAIT | EDGES | EXACT, 0, {})]
OVERFLOW = [("%s q=%d" % ("small" if fl else "grown", q), ALL, fl, {"wait_queue": q}) for q in (1, 5, 64)
            for fl in (0, SMALL)]
PLAN_LAUNCHES = dict(steps=1500, launches=(700, 1))
OVF_LAUNCHES = dict(steps=2000, launches=(7, 300))

CASES = [
    _case("sec11", G.sec11_graph, "plan", [EVERY], **PLAN_LAUNCHES),
    _case("grid48x48", functools.partial(grid, 48, 48), "plan", [EVERY] + SUBSETS, **PLAN_LAUNCHES),
    _case("grid70x70", functools.partial(grid, 70, 70), "plan", [EVERY], **PLAN_LAUNCHES),
    _case("grid104x104", functools.partial(grid, 104, 104), "plan", [EVERY], **PLAN_LAUNCHES),
    _case("grid160x128", functools.partial(grid, 160, 128), "plan", [EVERY], **PLAN_LAUNCHES),
    _case("grid144x144", functools.partial(grid, 144, 144), "plan", [EVERY], **PLAN_LAUNCHES),
    _case("delaunay7000", delaunay7000, "ring16", [EVERY], plans=strips, **PLAN_LAUNCHES),
    _case("ovf delaunay_wide", delaunay_wide, "overflow", OVERFLOW, plans=strips, bounds=FC.pct_bounds(0.9),
          bases=(1.0, 0.5, 2.0, 1.0), **OVF_LAUNCHES),
    _case("ovf grid9x7_weighted", FC.small_weights_grid, "overflow", OVERFLOW, plans=both_strips,
          bounds=FC.around_start(40), bases=(1.0, 0.7, 1.5), **OVF_LAUNCHES),
    _case("ovf grid48x48", functools.partial(grid, 48, 48), "overflow", OVERFLOW, **OVF_LAUNCHES),
    # a queued state's whole run in one entry (queue 64) / start-state entries of one batch each (1)
    _case("long grid6x6", functools.partial(grid, 6, 6), "long",
          [("q=64", ALL, 0, {"wait_queue": 64}), ("q=1", ALL, 0, {"wait_queue": 1})], bases=(2.0e4,), steps=3000000,
          launches=(), chain_ok=long_runs, want_events=True),
    _case("edge 2^23", functools.partial(grid, 4, 4), "edge", [EVERY], bases=(1.0, 2.0), n_chains=2, steps=1 << 23,
          launches=(), chain_ok=late_flips, slow=True),
    _case("edge 2^23+5", functools.partial(grid, 4, 4), "edge", [EVERY], bases=(1.0, 2.0), n_chains=2,
          steps=(1 << 23) + 5, launches=(), chain_ok=late_flips, slow=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(BY_NAME) & set(FC.BY_NAME)

# The hand-written plan table (limit 163,840, every tally): passes as (LDS mask, bytes), global mask.
SIX = [NF, PS, LF, FCN, OCC, LA]
HAND_PLANS = {
    "sec11": ([(511, 139248)], 0),  # n 1,596, E 3,116: 8 (2 E + 1) + 8 (7 n + 1)
    "grid48x48": ([(CUT | NB | EDGE | NF | PS | LF, 145936), (FCN | OCC | LA, 55296)], 0),
    "grid70x70": ([(CUT | NB | NF, 155696), (EDGE | PS | LF, 155680), (FCN | OCC | LA, 117600)], 0),
    "grid104x104": ([(NB, 86536)] + [(a, 86528) for a in SIX], CUT | EDGE),
    "grid160x128": ([(a, 163840) for a in SIX], CUT | NB | EDGE),
    "grid144x144": ([(0, 0)], 511),
}


# ---- the native plan program (tests/native/tally_plan_check.cpp) -----------------------------------
def build_plan_check(out_dir):
    """Compiles the program; None without a host C++ toolchain."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(str(out_dir), "tally_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "native", "tally_plan_check.cpp")], check=True)
    return exe


def native_plan(exe, diag, n, n_edges, limit):
    """plan_tally_reduce(diag, n, n_edges, limit) as FlipRun.tally_plan() reports a plan."""
    res = subprocess.run([exe, "plan", str(diag), str(n), str(n_edges), str(limit)], capture_output=True, text=True,
                         timeout=60, check=True)
    w = res.stdout.split()
    assert w[0] == "limit" and w[2] == "gmask" and w[4] == "passes", res.stdout
    k = int(w[5])
    assert len(w) == 6 + 2 * k, res.stdout
    return {"limit": int(w[1]), "passes": [(int(w[6 + 2 * i]), int(w[7 + 2 * i])) for i in range(k)],
            "global_mask": int(w[3])}
