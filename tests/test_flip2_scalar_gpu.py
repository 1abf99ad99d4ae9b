"""The lean k = 2 flip kernel's wave-uniform lane ranges and re-read launch parameters against the
C oracle.

The three lean node-stream 8-cell instances form their lane ranges (``csrc/fc_lane_mask.h``) with
shifts in place of a subtract and two selects, and read the issue-priority parameters and the
wait queue's seeds again from the kernel-argument segment where those rare blocks run.  What can go
wrong there is at the edges: a range that ends at lane 63 or 64 (a window closed by its 64th hit:
``ns = 64``, ``end = 64``), an empty range (``lo = hi``, few slots), the launch's last step inside a
segment pass or among the steps before a one-event commit (``kth_set_bit``, ``m_upto``), verdicts
that change inside a segment.  So:

* ``grid9x7`` and ``grid8x8`` at bases 0.1, 1 and 10 -- most nodes are boundary nodes, so nearly every
  window closes on its 64th hit; few, some and many acceptances: one-event commits, both
  re-evaluations, segment passes;
* ``grid3x3`` and ``cycle3`` -- 9 and 3 nodes, every draw a hit, batches of few steps at a launch's
  end, empty ranges;
* ``grid9x7_weighted`` -- population verdicts that change inside a segment;
* each in one launch and in three, whose ends (8 to 12 chains x 3 bases x 3 launches) fall inside
  segment passes at the high base and before a one-event commit at the low one;
* sec11 from its three start plans, 64 chains x 5,000 steps at the ten bases of the sweep.

Each run is compared with ``oracle/flipref.c`` chain by chain (``test_flip_edges_gpu._check``: every
statistic, the final assignment, the populations), and the kernel's name is the lean instance's.
The three-launch cases also run with ``tune ring_table=0``: the instance's second body.
"""
import dataclasses
import functools

import pytest

import flip_cases as FC
from flipcomplexityempirical_amd import graphs as G
from oracle.flipref import STREAM_NODE
from test_flip_edges_gpu import LEAN, _check, _run

pytestmark = pytest.mark.gpu

LEAN_NAME = "fc::flip2_kernel<8, 4, false, false, false, false>"
BASES = (0.1, 1.0, 10.0)
NAMES = ("grid9x7", "grid8x8", "grid3x3", "cycle3", "grid9x7_weighted")
K2 = [c for c in FC.K2_CASES if c.name in NAMES]
assert sorted(c.name for c in K2) == sorted(NAMES)


@functools.lru_cache(maxsize=None)
def _sec11():
    return G.sec11_graph()


def _sec11_plans(spec, k):
    return [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]


_ORACLE = {}


@dataclasses.dataclass(frozen=True)
class ScalarCase(FC.Case):
    """A case of this file, with its own oracle cache (flip_cases' names keep their coverage
    conditions in test_flip_cases.py; these have none of their own)."""

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
    kw.update(name=f"scalar {case.name} {tag}", bases=BASES, launches=launches, band=False)
    return _register(ScalarCase(**kw))


# (odd launch lengths: the ends fall at other places of their batches than a round number's)
CASES = [_derive(c, l) for c in K2 for l in ((), (c.steps // 3 + 1, c.steps // 4 + 7))]
CASES.append(_register(ScalarCase("scalar sec11", _sec11, 2, _sec11_plans, FC.pct_bounds(0.1), FC.all_steps,
                                  bases=tuple(G.SEC11_BASES), steps=5000, launches=(), n_chains=64, max_draws=50000000,
                                  trace_cap=0)))


# The lean instance carries its body twice and both got the changes: the list body with the ring table
# (these graphs have no node of more than four neighbours) runs every case; `tune ring_table=0` sends
# the run through the ring body, which runs the three-launch cases.
PARAMS = [(c, {}) for c in CASES] + [(c, {"ring_table": 0}) for c in CASES if c.launches]


@pytest.mark.parametrize("case,tune", PARAMS, ids=lambda x: x.name if isinstance(x, FC.Case) else ("ring body" if x else "list body"))
def test_lean_instance_equals_oracle(gpu, case, tune):
    assert 8 <= case.n_chains <= 64 and 2000 <= case.steps <= 5000
    fg, run = _run(case, LEAN, tune)
    assert fg.info["ring_max"] == 8 and fg.info["n_exact"] == fg.n
    assert run.kernel_name() == LEAN_NAME
    assert run.ring_table()["in_use"] == (0 if tune else 1)
    _check(case, run, LEAN)
    run.close()
    fg.close()
