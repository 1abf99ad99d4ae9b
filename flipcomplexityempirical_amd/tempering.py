"""Replica exchange (parallel tempering) over the chains of one run (DESIGN.md "Replica exchange").

The reference's result is that the flip walk mixes torpidly once ``base`` leaves 1; the standard
remedy is a ladder of bases run side by side whose neighbouring rungs trade temperatures with the
Metropolis swap probability.  A :class:`~flipcomplexityempirical_amd.engine.FlipRun` with per-chain
bases is such a ladder already; ``fc_run_exchange`` is the swap, a small device step between two
flip launches.  :class:`TemperedRun` lays out L ladders of m rungs, drives ``steps; exchange`` rounds
without host synchronisation, and reads the statistics per rung (per temperature), not per replica.
"""
from __future__ import annotations

from dataclasses import replace
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .engine import FlipGraph, FlipRun, RunConfig


def geometric_ladder(b_lo: float, b_hi: float, m: int) -> np.ndarray:
    """``m`` bases from ``b_lo`` to ``b_hi`` with a constant ratio between neighbours (equal swap
    odds per unit of |cut| difference along the ladder)."""
    if m < 1 or not (b_lo > 0 and b_hi > 0):
        raise ValueError("geometric_ladder needs m >= 1 and positive bases")
    if m == 1:
        return np.asarray([float(b_lo)])
    out = float(b_lo) * (float(b_hi) / float(b_lo)) ** (np.arange(m) / (m - 1))
    out[0], out[-1] = b_lo, b_hi
    return out


def swap_threshold(b_lo_rung: float, b_hi_rung: float, d: int) -> int:
    """The U53 threshold of one swap decision (``fc_ladder_swap_threshold``): the code the device
    runs.  ``d`` = |cut| of the lower rung's replica minus |cut| of the upper rung's."""
    import ctypes
    t = ctypes.c_uint64(0)
    _lib.check(_lib.load().fc_ladder_swap_threshold(float(b_lo_rung), float(b_hi_rung), int(d), ctypes.byref(t)),
               "fc_ladder_swap_threshold")
    return int(t.value)


class TemperedRun:
    """``L`` ladders of ``m`` rungs in one run: chain ``l * m + r`` starts from ``plans[l]`` at
    ``bases[r]``.  ``plans`` is ``[L, n]`` district ids (or ``[n]`` with ``n_ladders``)."""

    def __init__(self, graph: FlipGraph, plans: np.ndarray, bases: Sequence[float], cfg: RunConfig,
                 n_ladders: Optional[int] = None, hist: bool = False):
        a = np.asarray(plans, dtype=np.int8)
        if a.ndim == 1:
            a = np.broadcast_to(a, (n_ladders or 1, a.shape[0]))
        self.bases = np.asarray(bases, dtype=np.float64).reshape(-1)
        self.L, self.m = int(a.shape[0]), int(self.bases.size)
        if hist:
            cfg = replace(cfg, diag_mask=cfg.diag_mask | _lib.FC_DIAG_HIST)
        self.hist = bool(hist)
        self.run = FlipRun(graph, np.repeat(a, self.m, axis=0), cfg, bases=np.tile(self.bases, self.L))
        self.run.set_ladders([np.arange(l * self.m, (l + 1) * self.m) for l in range(self.L)], hist=hist)
        self.rounds = 0

    def advance(self, rounds: int, steps: int) -> "TemperedRun":
        """``rounds`` times: ``steps`` valid steps of every chain, then one exchange round (the
        round counter's parity).  Everything is enqueued; nothing waits for the device."""
        for _ in range(int(rounds)):
            self.run.steps(int(steps))
            self.run.exchange()
        self.rounds += int(rounds)
        return self

    def results(self) -> Dict[str, np.ndarray]:
        """Per rung, summed over the ladders: ``yields``, ``mean_cut`` / ``mean_nb`` over yields,
        the wait-weighted sums ``sum_wait``, ``sum_cut``, ``sum_nb``, ``swap_acceptance`` per
        adjacent pair ``[m - 1]``, and with ``hist`` the |cut| histogram ``[m, E + 1]``."""
        rs = self.run.rung_stats()
        per = {f: rs[f].reshape(self.L, self.m).sum(axis=0) for f, _ in _lib.RungStats._fields_}
        yields = per["steps"] + self.L  # every slot also got the initial yield of the chain listed there
        tried = per["swaps_tried"][:-1]
        out = {"bases": self.bases.copy(), "yields": yields,
               "mean_cut": per["sum_cut"] / yields, "mean_nb": per["sum_nb"] / yields,
               "sum_cut": per["sum_cut"], "sum_nb": per["sum_nb"], "sum_wait": per["sum_wait"],
               "swaps_tried": tried, "swaps_accepted": per["swaps_accepted"][:-1],
               "swap_acceptance": per["swaps_accepted"][:-1] / np.maximum(tried, 1)}
        if self.hist:
            out["cut_hist"] = rs["cut_hist"].reshape(self.L, self.m, -1).sum(axis=0)
            out["nb_hist"] = rs["nb_hist"].reshape(self.L, self.m, -1).sum(axis=0)
        return out

    def close(self):
        self.run.close()
