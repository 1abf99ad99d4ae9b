"""flip2_kernel's ring-verdict table (``csrc/fc_ring_table.h``) against the C oracle and against the
arithmetic it replaces.

The lean node-stream instance of a graph without a node of more than four neighbours reads a slot's
verdicts -- boundary hit, the two run-rule verdicts, delta-cut, old-district neighbours -- from one
table entry per (ring class, ring byte), in phase 2 and in both re-evaluations of the commit.  What
can go wrong there: padded ring cells (rings shorter than 8: the index byte carries the node's own
district above the ring length), outer-face nodes (where the closed-ring verdict decides), a view
updated in registers after a one-event commit or re-read after a segment pass, and the fall-back to
the arithmetic when the graph has more classes than the cap.  So every k = 2 case of
``flip_cases`` that launches the lean instance runs here at bases 0.1, 1 and 10 (few, some and many
rejections: one-event commits, both re-evaluations, segment passes), in one launch and in three, and
sec11 runs from its three start plans; each run is compared with ``oracle/flipref.c`` chain by chain
(``test_flip_edges_gpu._check``: every statistic, the final assignment, the populations), and with
the same run under ``tune ring_table=0``, which must leave the same bytes.
"""
import dataclasses
import functools

import numpy as np
import pytest

import flip_cases as FC
from flipcomplexityempirical_amd import graphs as G
from oracle.flipref import STREAM_NODE
from test_flip_edges_gpu import LEAN, _check, _run

pytestmark = pytest.mark.gpu

LEAN_NAME = "fc::flip2_kernel<8, 4, false, false, false, false>"
BASES = (0.1, 1.0, 10.0)


# the k = 2 cases of flip_cases that launch the lean instance (every ring exact and of at most 8
# cells): the grids and the triangle `cycle3` -- rings of 2 cells, six padded cells in the index byte,
# every node on the outer face, the closing link at its shortest.  The other paths and cycles and
# `all_accept` have no exact ring: they launch the search instance, which keeps the arithmetic.
# Chosen by name, so that collecting this file builds no graph; each test asserts what the choice
# assumes on the built graph.
LEAN_CASES = ("grid3x3", "grid4x4", "grid4x4_heavy", "grid9x7", "grid9x7_weighted", "grid8x8", "cycle3")
K2 = [c for c in FC.K2_CASES if c.name in LEAN_CASES]
assert [c.name for c in K2] == list(LEAN_CASES)


@functools.lru_cache(maxsize=None)
def _sec11():
    return G.sec11_graph()


def _sec11_plans(spec, k):
    return [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]


_ORACLE = {}


@dataclasses.dataclass(frozen=True)
class TableCase(FC.Case):
    """A case of this file: its oracle runs are cached here, not under flip_cases' names (whose
    cases test_flip_cases.py holds to their coverage conditions; these have none of their own)."""

    def oracle(self, c, stream=STREAM_NODE):
        key = (self.name, c, stream)
        if key not in _ORACLE:
            lo, hi = self.chain_bounds(c)
            _ORACLE[key] = FC._cref().run(self.spec, self.plan(c), base=self.base(c), pop_lo=lo, pop_hi=hi, seed=self.seed,
                                          chain_id=c, n_steps=self.steps, k=self.k, labels=list(self.labels),
                                          log1mp=G.log1mp_table(self.spec.n, self.k), max_draws=self.max_draws,
                                          stream=stream)
        return _ORACLE[key]


BY_NAME = {}


def _register(c):
    assert BY_NAME.setdefault(c.name, c) is c
    return c


def _derive(case, launches):
    """`case` at the three bases, in one launch (launches = ()) or three."""
    tag = "3 launches" if launches else "1 launch"
    kw = {f.name: getattr(case, f.name) for f in dataclasses.fields(case)}
    kw.update(name=f"ring table {case.name} {tag}", bases=BASES, launches=launches, band=False)
    return _register(TableCase(**kw))


CASES = [_derive(c, l) for c in K2 for l in ((), (c.steps // 3, c.steps // 4))]
# sec11 from its three start plans, dealt round-robin, at the ten bases of the sweep
CASES.append(_register(TableCase("ring table sec11", _sec11, 2, _sec11_plans, FC.pct_bounds(0.1), FC.all_steps,
                               bases=tuple(G.SEC11_BASES), steps=5000, launches=(), n_chains=64, max_draws=50000000,
                               trace_cap=0)))


def _snapshot(run):
    st = run.stats()
    return {k: np.asarray(v).copy() for k, v in st.items()}, run.state().copy(), run.pops().copy()


def _same(a, b, who):
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), f"{who}: stat {key} differs between the table and the arithmetic"
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), who


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_table_equals_oracle_and_arithmetic(gpu, case):
    assert 8 <= case.n_chains <= 64 and 2000 <= case.steps <= 5000
    snaps = []
    for tune, used in (({}, 1), ({"ring_table": 0}, 0)):
        fg, run = _run(case, LEAN, tune)
        assert fg.info["ring_max"] == 8 and fg.info["n_exact"] == fg.n
        assert run.kernel_name() == LEAN_NAME
        rt = run.ring_table()
        assert rt["in_use"] == used and 1 <= rt["classes"] <= 64, rt
        _check(case, run, LEAN)
        snaps.append(_snapshot(run))
        run.close()
        fg.close()
    _same(snaps[0], snaps[1], case.name)


def test_cap_at_the_class_count_and_one_below(gpu):
    """9 x 7 grid: with the cap at the graph's class count the table is read, with one less the run
    falls back to the arithmetic; both are the oracle's chain."""
    case = BY_NAME["ring table grid9x7 3 launches"]
    fg, run = _run(case, LEAN, {})
    classes = run.ring_table()["classes"]
    run.close()
    fg.close()
    assert classes >= 2
    snaps = []
    for cap, used in ((classes, 1), (classes - 1, 0)):
        fg, run = _run(case, LEAN, {"ring_table": cap})
        assert run.kernel_name() == LEAN_NAME
        assert run.ring_table() == {"classes": classes, "in_use": used}
        _check(case, run, LEAN)
        snaps.append(_snapshot(run))
        run.close()
        fg.close()
    _same(snaps[0], snaps[1], case.name)
