"""Optimization by short bursts on the device: ``gerrychain.optimization``'s
``SingleMetricOptimizer.short_bursts`` for ReCom chains, many chains at once.

A burst is ``burst_length`` steps of every chain (one launch); after it the device scores every
yield of the burst by the metric, keeps the latest yield with the best score and restarts the
chain from the plan it held there (``FlipRun.burst_select(..., rewind=True)``): no plan is read
back to the host between bursts.

The metric objects are built from :class:`~flipcomplexityempirical_amd.chain.Election`, whose
columns reach the run by the path ``MarkovChain._set_series_updaters`` uses, and each is also
callable on a :class:`~flipcomplexityempirical_amd.chain.Partition`: the Python definition the
device's score is checked against.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Dict, List

import numpy as np

from . import _lib
from .chain import Election, Partition, compile_chain
from .engine import BurstMetric, FlipGraph, FlipRun, RunConfig
from .graphs import node_columns


class DistrictCount:
    """The number of districts in which ``party``'s share of the two-party vote of ``election`` is
    above ``threshold`` (1/2: the party's seats; another fraction: the districts above a share).
    Equality does not count."""

    def __init__(self, election: Election, party, threshold=Fraction(1, 2)):
        if party not in election.parties:
            raise KeyError(party)
        self.election, self.party = election, party
        self.threshold = Fraction(threshold)
        if not 0 < self.threshold < 1 or self.threshold.denominator > 2 ** 20:
            raise ValueError("threshold must be a fraction in (0, 1) with a denominator of at most 2^20")

    def columns(self) -> List[str]:
        """The node columns (a, b): the party's and the other party's."""
        cols = self.election.parties_to_columns
        other = next(p for p in self.election.parties if p != self.party)
        return [cols[self.party], cols[other]]

    def device(self, col_a: int, col_b: int, maximize: bool) -> BurstMetric:
        return BurstMetric("count", col_a, col_b, self.threshold.numerator, self.threshold.denominator, maximize)

    def __call__(self, partition) -> int:
        res = self.election(partition)
        other = next(p for p in self.election.parties if p != self.party)
        num, den = self.threshold.numerator, self.threshold.denominator
        return sum(1 for part in res.parts
                   if den * int(res.totals_for_party[self.party][part]) >
                   num * (int(res.totals_for_party[self.party][part]) + int(res.totals_for_party[other][part])))


class EfficiencyGap:
    """|wasted votes of the second party - wasted votes of the first| in doubled integer units:
    ``|sum over the districts of g(a, b)|`` with ``g = 3b - a`` (a > b), ``b - 3a`` (a < b), 0 (a
    tie); divided by twice the election's votes it is ``|ElectionResults.efficiency_gap()|``."""

    def __init__(self, election: Election):
        self.election = election

    def columns(self) -> List[str]:
        return list(self.election.columns)

    def device(self, col_a: int, col_b: int, maximize: bool) -> BurstMetric:
        return BurstMetric("gap", col_a, col_b, 1, 2, maximize)

    def __call__(self, partition) -> int:
        res = self.election(partition)
        pa, pb = self.election.parties
        g = 0
        for part in res.parts:
            a, b = int(res.totals_for_party[pa][part]), int(res.totals_for_party[pb][part])
            g += 3 * b - a if a > b else (b - 3 * a if a < b else 0)
        return abs(g)


class CutEdges:
    """The number of cut edges."""

    def columns(self) -> List[str]:
        return []

    def device(self, col_a: int, col_b: int, maximize: bool) -> BurstMetric:
        return BurstMetric("cut", 0, 1, 1, 2, maximize)

    def __call__(self, partition) -> int:
        return len(partition["cut_edges"])


class SingleMetricOptimizer:
    """``gerrychain.optimization.SingleMetricOptimizer`` for the device: ``n_chains`` independent
    ReCom chains from ``initial_state`` (chain ids ``0 .. n_chains - 1`` of ``seed``), every proposal
    accepted, optimised by short bursts.  ``optimization_metric`` is a :class:`DistrictCount`,
    :class:`EfficiencyGap` or :class:`CutEdges`."""

    def __init__(self, proposal, constraints, initial_state: Partition, optimization_metric, maximize: bool = True,
                 n_chains: int = 1, seed: int = 0, device: int = 0):
        from .chain import always_accept
        if not all(hasattr(optimization_metric, a) for a in ("columns", "device")):
            raise TypeError("optimization_metric must be a DistrictCount, EfficiencyGap or CutEdges")
        self.cspec = compile_chain(proposal, constraints, always_accept, initial_state)
        if self.cspec.proposal != _lib.FC_PROPOSE_RECOM:
            raise NotImplementedError("short bursts restart a chain from the best plan of its burst, and the device "
                                      "rewinds ReCom chains only (a flip chain keeps derived per-node state a rewind "
                                      "would have to rebuild): give a partial(recom, ...) proposal")
        self.initial_state, self.metric, self.maximize = initial_state, optimization_metric, bool(maximize)
        self.n_chains, self.seed, self.device = int(n_chains), int(seed), int(device)
        self._graph = None
        self.best_score = None
        self.best_part = None

    def _make_run(self, burst_length: int) -> FlipRun:
        cs = self.cspec
        if self._graph is None:
            self._graph = FlipGraph(cs.spec)
        k, n = len(cs.labels), cs.spec.n
        # a step moves at most n nodes, so a burst's log never overflows; a chunk of margin
        cfg = RunConfig(k=k, labels=tuple(cs.dev_labels if cs.dev_labels is not None else range(k)),
                        proposal=cs.proposal, seed=self.seed, pop_lo=cs.pop_lo, pop_hi=cs.pop_hi, base=cs.base,
                        device=self.device, diag_mask=_lib.FC_DIAG_SERIES, event_cap=int(burst_length) * n + 64,
                        recom_pop_target=cs.recom["pop_target"], recom_epsilon=cs.recom["epsilon"],
                        recom_node_repeats=cs.recom["node_repeats"])
        run = FlipRun(self._graph, np.broadcast_to(cs.init, (self.n_chains, n)), cfg)
        names = self.metric.columns()
        if names:
            cols = node_columns(self.initial_state.graph, cs.spec.nodes, names)
            run.set_elections(np.stack([cols[c] for c in names], axis=1), [(0, 1)])
        self._metric = self.metric.device(0, 1, self.maximize)
        return run

    def partition(self, assignment_row) -> Partition:
        """The :class:`Partition` of one row of ``best_part`` (district indices in node order)."""
        cs = self.cspec
        return Partition(self.initial_state.graph,
                         {nd: cs.labels[int(d)] for nd, d in zip(cs.spec.nodes, assignment_row)},
                         self.initial_state.updaters)

    def short_bursts(self, burst_length: int, num_bursts: int) -> Dict[str, np.ndarray]:
        """``num_bursts`` bursts of ``burst_length`` steps.  Returns ``best_score`` ``[n_chains]``,
        ``best_part`` int8 ``[n_chains, n]`` (district indices in node order; :meth:`partition`
        makes a Partition of a row) and ``score_trace`` ``[num_bursts, n_chains]``, each chain's
        best score after every burst: monotone, since the plan a burst starts from is a candidate."""
        if int(burst_length) < 1 or int(num_bursts) < 1:
            raise ValueError("burst_length and num_bursts must be at least 1")
        run = self._make_run(burst_length)
        trace = np.zeros((int(num_bursts), self.n_chains), dtype=np.int64)
        try:
            for i in range(int(num_bursts)):
                run.steps(int(burst_length))
                trace[i] = run.burst_select(self._metric, rewind=True)["best_score"]
            # every chain now stands on its best plan
            self.best_part = run.state()
        finally:
            run.close()
        self.best_score = trace[-1].copy()
        return {"best_score": self.best_score, "best_part": self.best_part, "score_trace": trace}
