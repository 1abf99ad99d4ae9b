"""Batched multi-chain engine over the C-ABI: the MI355X replacement of the reference's
``Partition`` + ``MarkovChain`` hot loop (``grid_chain_sec11.py:316-408``).

``FlipGraph`` owns an ``fc_graph`` (CSR + link rings, built natively from a
:class:`~flipcomplexityempirical_amd.graphs.GraphSpec`); ``FlipRun`` owns an ``fc_run``
(``n_chains`` independent k=2 chains, one per wavefront on the device).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check
from .graphs import GraphSpec, log1mp_table, nb_width

_P = ctypes.POINTER

STAT_FIELDS = [f for f, _ in _lib.ChainStats._fields_]
RECORD_DTYPE = np.dtype([("draw", "<i8"), ("v", "<i4"), ("flags", "<i4"), ("cut", "<i4"),
                         ("nb", "<i4"), ("wait", "<i8")])
RECOM_RECORD_DTYPE = np.dtype([("draw", "<i8"), ("edge", "<i4"), ("root", "<i4"), ("child", "<i4"),
                               ("attempts", "<i4"), ("flags", "<i4"), ("cut", "<i4")])
EVENT_DTYPE = np.dtype([("t", "<i8"), ("v", "<u2"), ("cut", "<u2"), ("nb", "<u2"), ("target", "u1"),
                        ("reserved", "u1")])


def _p(arr, ct):
    return arr.ctypes.data_as(_P(ct)) if arr is not None else _P(ct)()


def _set_fields(struct, **fields):
    for name, val in fields.items():
        setattr(struct, name, val)


def pin_host(arr: np.ndarray) -> np.ndarray:
    """Page-lock a numpy buffer for the device-to-host copies of the readers
    (``fc_host_register``); :func:`unpin_host` before it is freed."""
    check(_lib.load().fc_host_register(ctypes.c_void_p(arr.ctypes.data), int(arr.nbytes)), "fc_host_register")
    return arr


def unpin_host(arr: np.ndarray) -> None:
    check(_lib.load().fc_host_unregister(ctypes.c_void_p(arr.ctypes.data)), "fc_host_unregister")


def sample_times(t0: int, t_last: int, every: int, first: Optional[int] = None) -> np.ndarray:
    """The yields ``first`` (``t0`` when None), ``+ every``, ... up to ``t_last`` inclusive, int64:
    the times of :meth:`FlipRun.sample_plans` for a window of yields ``t0 .. t_last``."""
    if int(every) < 1:
        raise ValueError("every must be at least 1")
    start = int(t0) if first is None else int(first)
    return np.arange(start, int(t_last) + 1, int(every), dtype=np.int64)


BURST_KINDS = {"count": _lib.FC_BURST_COUNT, "gap": _lib.FC_BURST_GAP, "cut": _lib.FC_BURST_CUT}


@dataclass(frozen=True)
class BurstMetric:
    """A short-bursts metric (``fc_burst_metric``; include/flipchain.h): ``kind`` "count" (the
    districts with ``den * a > num * (a + b)``), "gap" (|efficiency gap| in doubled integer units)
    or "cut" (|cut|); ``col_a`` / ``col_b`` columns of :meth:`FlipRun.set_elections` (vote kinds)."""
    kind: str = "cut"
    col_a: int = 0
    col_b: int = 1
    num: int = 1
    den: int = 2
    maximize: bool = True

    def struct(self) -> "_lib.BurstMetric":
        m = _lib.BurstMetric()
        check(_lib.load().fc_burst_metric_init(ctypes.byref(m), ctypes.sizeof(_lib.BurstMetric)), "fc_burst_metric_init")
        kind = BURST_KINDS.get(self.kind, self.kind)
        if not isinstance(kind, int):
            raise ValueError(f"unknown metric kind {self.kind!r} (known: {', '.join(BURST_KINDS)})")
        _set_fields(m, kind=kind, col_a=int(self.col_a), col_b=int(self.col_b), num=int(self.num), den=int(self.den),
                    maximize=int(self.maximize))
        return m

    def eval(self, a=None, b=None, cut: int = 0) -> int:
        """The score of one state by the rule the device applies (``fc_burst_eval``; no GPU):
        ``a`` / ``b`` ``[k]`` the districts' tallies of the two columns, ``cut`` its |cut|."""
        a = None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.int64)
        if (a is None) != (b is None) or (a is not None and (a.ndim != 1 or a.shape != b.shape)):
            raise ValueError("a and b must be two [k] arrays")
        k = 1 if a is None else int(a.size)
        m, score = self.struct(), ctypes.c_int64(0)
        check(_lib.load().fc_burst_eval(ctypes.byref(m), k, _p(a, ctypes.c_int64), _p(b, ctypes.c_int64), int(cut),
                                        ctypes.byref(score)), "fc_burst_eval")
        return int(score.value)


class FlipGraph:
    """Native graph handle (``fc_graph_create``)."""

    def __init__(self, spec: GraphSpec, use_positions: bool = True, exact: bool = True):
        self.spec = spec
        L = _lib.load()
        self._row = np.ascontiguousarray(spec.row_ptr, dtype=np.int32)
        self._col = np.ascontiguousarray(spec.col_idx, dtype=np.int32)
        self._pop = np.ascontiguousarray(spec.pop, dtype=np.int32)
        pos = None
        if use_positions and spec.pos is not None:
            pos = np.ascontiguousarray(spec.pos, dtype=np.float64).reshape(-1)
        h = ctypes.c_void_p()
        flags = 0 if exact else _lib.FC_GRAPH_NO_EXACT
        check(L.fc_graph_create(spec.n, _p(self._row, ctypes.c_int32), _p(self._col, ctypes.c_int32),
                                _p(self._pop, ctypes.c_int32), _p(pos, ctypes.c_double), flags,
                                ctypes.byref(h)), "fc_graph_create")
        self.handle = h
        info = _lib.GraphInfo()
        check(L.fc_graph_get_info(h, ctypes.byref(info)), "fc_graph_get_info")
        self.info = {f: getattr(info, f) for f, _ in _lib.GraphInfo._fields_}

    @property
    def n(self) -> int:
        return self.info["n_nodes"]

    @property
    def n_edges(self) -> int:
        return self.info["n_edges"]

    def edges(self) -> np.ndarray:
        eu = np.zeros(self.n_edges, dtype=np.int32)
        ev = np.zeros(self.n_edges, dtype=np.int32)
        check(_lib.load().fc_graph_edges(self.handle, _p(eu, ctypes.c_int32), _p(ev, ctypes.c_int32)))
        return np.stack([eu, ev], axis=1)

    def rings(self):
        R = self.info["ring_max"]
        ring = np.zeros(self.n * R, dtype=np.int32)
        meta = np.zeros(self.n, dtype=np.uint64)
        check(_lib.load().fc_graph_rings(self.handle, _p(ring, ctypes.c_int32), _p(meta, ctypes.c_uint64)))
        return ring.reshape(self.n, R), meta

    def heat_rows(self):
        """``(nbr, eid)``, ``[n, width]`` each: the neighbour / edge rows the heat-map replay walks
        (``fc_graph_heat_rows``; host code, no device): slot j of node u holds a neighbour and the
        canonical id of the edge to it, -1 / -1 when empty."""
        L = _lib.load()
        width = ctypes.c_int32(0)
        check(L.fc_graph_heat_rows(self.handle, ctypes.byref(width), None, None), "fc_graph_heat_rows")
        nbr = np.zeros(self.n * width.value, dtype=np.int32)
        eid = np.zeros(self.n * width.value, dtype=np.int32)
        check(L.fc_graph_heat_rows(self.handle, ctypes.byref(width), _p(nbr, ctypes.c_int32), _p(eid, ctypes.c_int32)),
              "fc_graph_heat_rows")
        return nbr.reshape(self.n, width.value), eid.reshape(self.n, width.value)

    def seed_plans(self, k: int, n_plans: int, *, pop_bounds=None, percent: Optional[float] = None, seed: int = 0,
                   plan_id_offset: int = 0, node_repeats: int = 1, max_attempts: int = 0, max_restarts: int = 0,
                   strict: bool = True, device: int = 0, timing: bool = False):
        """``n_plans`` random k-district start plans by recursive spanning-tree bipartition on the
        device (``fc_graph_seed_plans``, gerrychain's ``recursive_tree_part``):
        ``(plans, stats)`` with ``plans`` int8 ``[n_plans, n]`` (district ids 0..k-1 in canonical
        node order, one row per chain of ``FlipRun``) and ``stats`` the per-plan ``attempts``,
        ``trees``, ``restarts``, ``ok``, ``cut`` and ``nb`` arrays, plus ``kernel`` (the launched
        instance) and, with ``timing``, ``kernel_ms``.

        The districts' inclusive integer population bounds are ``pop_bounds=(lo, hi)``, or
        ``percent`` through :func:`graphs.population_bounds` -- give exactly one.  Plan ``i`` is the
        plan of global id ``plan_id_offset + i`` under ``seed``: it does not depend on the call it
        is computed in, so ranks that pass disjoint id ranges share one ensemble.  A plan that
        found no cut within ``max_attempts`` attempts per level (0: 256) in ``max_restarts``
        restarts (0: 16) has ``ok = 0`` and a row of -1: ``strict`` raises ``RuntimeError`` naming
        those ids, otherwise read ``stats["ok"]``."""
        from .graphs import population_bounds
        if (pop_bounds is None) == (percent is None):
            raise ValueError("seed_plans: give exactly one of pop_bounds=(lo, hi) and percent")
        if percent is not None:
            pop_bounds = population_bounds(int(self.spec.pop.astype(np.int64).sum()), int(k), float(percent))[1]
        lo, hi = (int(x) for x in pop_bounds)
        L = _lib.load()
        prm = _lib.SeedParams()
        check(L.fc_seed_params_init(ctypes.byref(prm), ctypes.sizeof(prm)), "fc_seed_params_init")
        _set_fields(prm, k=int(k), pop_lo=lo, pop_hi=hi, seed=int(seed), plan_id_offset=int(plan_id_offset),
                    device=int(device), node_repeats=int(node_repeats), max_attempts=int(max_attempts),
                    max_restarts=int(max_restarts))
        n_plans = int(n_plans)
        plans = np.zeros((max(n_plans, 0), self.n), dtype=np.int8)
        st = (_lib.SeedStats * max(n_plans, 1))()
        ms = ctypes.c_float(0.0)
        check(L.fc_graph_seed_plans(self.handle, ctypes.byref(prm), n_plans, _p(plans, ctypes.c_int8), st,
                                    ctypes.byref(ms) if timing else None), "fc_graph_seed_plans")
        stats: Dict[str, Any] = {f: np.asarray([getattr(st[i], f) for i in range(n_plans)], dtype=np.int64)
                                 for f, _ in _lib.SeedStats._fields_}
        name = ctypes.create_string_buffer(96)
        check(L.fc_seed_kernel_name(name, 96), "fc_seed_kernel_name")
        stats["kernel"] = name.value.decode()
        if timing:
            stats["kernel_ms"] = float(ms.value)
        failed = np.nonzero(stats["ok"] == 0)[0]
        if strict and len(failed):
            ids = ", ".join(str(int(plan_id_offset) + int(i)) for i in failed[:16]) + (", ..." if len(failed) > 16 else "")
            raise RuntimeError(f"seed_plans: {len(failed)} of {n_plans} plans found no cut within max_attempts / "
                               f"max_restarts (plan ids {ids}); widen the bounds or raise them, or pass strict=False "
                               "and read stats['ok']")
        return plans, stats

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().fc_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass


@dataclass
class RunConfig:
    k: int = 2
    base: float = 1.0
    pop_lo: int = 0
    pop_hi: int = 2 ** 31 - 1
    seed: int = 0
    chain_id_offset: int = 0
    diag_mask: int = _lib.FC_DIAG_WAIT
    flags: int = 0
    device: int = 0
    trace_chains: int = 0
    trace_cap: int = 0
    labels: Sequence[int] = (-1, 1)
    proposal: int = _lib.FC_PROPOSE_BI_SIGN
    wmax: int = 0
    hit_lo: int = 1          # hitting-time window on |cut| (hit_lo > hit_hi: off)
    hit_hi: int = 0
    event_cap: int = 0       # FC_DIAG_SERIES events kept per chain per window
    # accept / constraint variants (k = 2; defaults: Validator([contiguous, popbound]) + cut_accept)
    accept: int = _lib.FC_ACCEPT_CUT
    con_valid: int = 0       # FC_CON_* of the Validator (0: CONTIG | POP)
    con_accept: int = 0      # FC_CON_* tested by the accept callable
    beta: float = 0.0        # FC_ACCEPT_ANNEAL exponent factor
    frozen: Sequence[int] = ()  # FC_CON_FIXED: endpoints of the pinned edges
    # FC_PROPOSE_RECOM: recom(pop_target, epsilon, node_repeats) (grid_chain_sec11.py:328-335)
    recom_pop_target: float = 0.0
    recom_epsilon: float = 0.05
    recom_node_repeats: int = 1
    recom_max_attempts: int = 0
    # launch tuning (fc_params.tune_*): scheduling only, never the trajectory; 0 = default.
    # Keys: nsub, hit_stop, par_min, wait_queue, chains_per_block, prio_div (3), prio_th (3),
    # search_waves, deal, multi_flip, ring_table (0 = no table: a value there, the default is 64).
    tune: Optional[Dict[str, object]] = None
    # k = 2 node stream (fc_params.stream): "node" draws over all n nodes, "band" over the band
    # S = b_nodes + neighbours; the chain's law is the same, the trajectory not
    stream: str = "node"


TUNE_KEYS = ("nsub", "hit_stop", "par_min", "wait_queue", "chains_per_block", "prio_div", "prio_th",
             "search_waves", "deal", "multi_flip", "ring_table")


def parse_tune(text: str) -> Dict[str, object]:
    """``"nsub=2,hit_stop=24,prio_div=2:5:10"`` -> RunConfig.tune (tools / bench.py --tune)."""
    out: Dict[str, object] = {}
    for item in filter(None, (t.strip() for t in (text or "").split(","))):
        key, _, val = item.partition("=")
        if key not in TUNE_KEYS:
            raise ValueError(f"unknown tuning key {key!r} (known: {', '.join(TUNE_KEYS)})")
        if key in ("prio_div", "prio_th"):
            conv = int if key == "prio_div" else float
            vals = [conv(x) for x in val.split(":")]
            out[key] = tuple(vals) + (vals[-1],) * (3 - len(vals)) if len(vals) < 3 else tuple(vals[:3])
        else:
            out[key] = int(val)
    return out


class FlipRun:
    """``n_chains`` chains on one GPU (``fc_run_create``).  ``init_assign`` is
    ``[n_chains, n]`` (or ``[n]``, broadcast) district ids; ``bases`` optional per chain."""

    def __init__(self, graph: FlipGraph, init_assign: np.ndarray, cfg: RunConfig,
                 bases: Optional[Sequence[float]] = None, n_chains: Optional[int] = None,
                 log1mp: Optional[np.ndarray] = None, pop_bounds: Optional[np.ndarray] = None):
        """``pop_bounds`` (optional): ``[n_chains, 2]`` inclusive population bounds per chain
        (``fc_params.chain_pop_bounds``), so that configurations of different tolerance share a
        run; default ``cfg.pop_lo`` / ``cfg.pop_hi`` for every chain."""
        L = _lib.load()
        self.graph = graph
        self.cfg = cfg
        a = np.asarray(init_assign, dtype=np.int8)
        if a.ndim == 1:
            a = np.broadcast_to(a, (n_chains or 1, a.shape[0]))
        self.n_chains = int(a.shape[0])
        self._init = np.ascontiguousarray(a)
        if self._init.shape[1] != graph.n:
            raise ValueError("init_assign must have one entry per node")
        labels = list(cfg.labels) if len(cfg.labels) == cfg.k else list(range(cfg.k))
        self._labels = np.ascontiguousarray(labels, dtype=np.int32)
        pairs = bool(cfg.flags & _lib.FC_FLAG_NB_PAIRS) and cfg.k > 2
        width = nb_width(graph.spec, cfg.k, True) if pairs else graph.n + 1
        self._log1mp = np.ascontiguousarray(log1mp if log1mp is not None else log1mp_table(graph.n, cfg.k, width),
                                            dtype=np.float64)
        if self._log1mp.size < width:
            raise ValueError(f"log1mp needs {width} entries (|b_nodes| 0 .. {width - 1})")
        self._bases = None if bases is None else np.ascontiguousarray(bases, dtype=np.float64)
        if self._bases is not None and self._bases.shape[0] != self.n_chains:
            raise ValueError("bases must have one entry per chain")
        self._pop_bounds = None
        if pop_bounds is not None:
            self._pop_bounds = np.ascontiguousarray(pop_bounds, dtype=np.int64).reshape(-1)
            if self._pop_bounds.size != 2 * self.n_chains:
                raise ValueError("pop_bounds must be [n_chains, 2]")
        prm = _lib.Params()
        check(L.fc_params_init(ctypes.byref(prm), ctypes.sizeof(_lib.Params)), "fc_params_init")
        _set_fields(prm, k=cfg.k, proposal=int(cfg.proposal), base=float(cfg.base), wmax=int(cfg.wmax),
                    pop_lo=int(cfg.pop_lo), pop_hi=int(cfg.pop_hi), seed=int(cfg.seed),
                    chain_id_offset=int(cfg.chain_id_offset), diag_mask=int(cfg.diag_mask),
                    flags=int(cfg.flags), device=int(cfg.device), trace_chains=int(cfg.trace_chains),
                    trace_cap=int(cfg.trace_cap), labels=_p(self._labels, ctypes.c_int32),
                    log1mp=_p(self._log1mp, ctypes.c_double), hit_lo=int(cfg.hit_lo),
                    hit_hi=int(cfg.hit_hi), event_cap=int(cfg.event_cap), accept=int(cfg.accept),
                    con_valid=int(cfg.con_valid), con_accept=int(cfg.con_accept), beta=float(cfg.beta))
        prm.chain_pop_bounds = _p(self._pop_bounds, ctypes.c_int64)
        if cfg.stream not in ("node", "band"):
            raise ValueError(f"stream must be 'node' or 'band', not {cfg.stream!r}")
        prm.stream = _lib.STREAM_BAND if cfg.stream == "band" else _lib.STREAM_NODE
        self._frozen = np.ascontiguousarray(list(cfg.frozen), dtype=np.int32)
        prm.frozen = _p(self._frozen, ctypes.c_int32)
        prm.n_frozen = int(self._frozen.size)
        prm.recom_pop_target = float(cfg.recom_pop_target)
        prm.recom_epsilon = float(cfg.recom_epsilon)
        prm.recom_node_repeats = int(cfg.recom_node_repeats)
        prm.recom_max_attempts = int(cfg.recom_max_attempts)
        for key, val in (cfg.tune or {}).items():
            if key not in TUNE_KEYS:
                raise ValueError(f"unknown tuning key {key!r}")
            if key in ("prio_div", "prio_th"):
                arr = getattr(prm, "tune_" + key)
                for i, x in enumerate(val):
                    arr[i] = x
            else:
                setattr(prm, "tune_" + key, int(val))
        h = ctypes.c_void_p()
        check(L.fc_run_create(graph.handle, ctypes.byref(prm), self.n_chains, _p(self._init, ctypes.c_int8),
                              _p(self._bases, ctypes.c_double), ctypes.byref(h)), "fc_run_create")
        self.handle = h
        self._tape = None

    # ---- stepping ---------------------------------------------------------------------
    def steps(self, n_steps: int, max_draws: int = 0, stream: Optional[int] = None) -> "FlipRun":
        check(_lib.load().fc_run_steps(self.handle, int(n_steps), int(max_draws),
                                       ctypes.c_void_p(stream) if stream else None), "fc_run_steps")
        return self

    def set_tape(self, tape: Optional[np.ndarray], n_draws: int = 0):
        """Replay: ``tape`` is ``[n_chains, n_draws * 6]`` u32."""
        if tape is None:
            check(_lib.load().fc_run_set_tape(self.handle, _P(ctypes.c_uint32)(), 0))
            self._tape = None
            return
        t = np.ascontiguousarray(tape, dtype=np.uint32).reshape(self.n_chains, -1)
        n_draws = t.shape[1] // 6
        self._tape = t
        check(_lib.load().fc_run_set_tape(self.handle, _p(t, ctypes.c_uint32), n_draws), "fc_run_set_tape")

    def set_initial_wait(self, words: np.ndarray):
        """Replay the initial states' geometric waits: ``words`` is ``[n_chains, 2]`` u32 (the
        53-bit uniform numpy's geometric inverted; ``fc_run_set_initial_wait``)."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(self.n_chains, 2)
        check(_lib.load().fc_run_set_initial_wait(self.handle, _p(w, ctypes.c_uint32)), "fc_run_set_initial_wait")

    def checkpoint(self) -> bytes:
        """The run's resumable state as bytes (``fc_run_checkpoint``)."""
        L = _lib.load()
        n = ctypes.c_int64(0)
        check(L.fc_run_checkpoint(self.handle, None, 0, ctypes.byref(n)), "fc_run_checkpoint")
        buf = ctypes.create_string_buffer(int(n.value))
        check(L.fc_run_checkpoint(self.handle, buf, n.value, ctypes.byref(n)), "fc_run_checkpoint")
        return buf.raw

    def restore(self, blob: bytes):
        """Load a ``checkpoint()`` of a run with the same graph and configuration."""
        buf = ctypes.create_string_buffer(bytes(blob), len(blob))
        check(_lib.load().fc_run_restore(self.handle, buf, len(blob)), "fc_run_restore")

    def sync(self):
        check(_lib.load().fc_run_sync(self.handle))

    def last_ms(self) -> float:
        ms = ctypes.c_float(0)
        check(_lib.load().fc_run_last_ms(self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def timings(self, cap: int = 4096) -> np.ndarray:
        """Device ms of every launch since the previous call (HIP events on the run's stream)."""
        out = np.zeros(cap, dtype=np.float32)
        n = ctypes.c_int32(0)
        check(_lib.load().fc_run_timings(self.handle, _p(out, ctypes.c_float), cap, ctypes.byref(n)))
        return out[:min(n.value, cap)].astype(np.float64)

    # ---- readouts ---------------------------------------------------------------------
    def stats(self) -> Dict[str, np.ndarray]:
        arr = (_lib.ChainStats * self.n_chains)()
        check(_lib.load().fc_run_read_stats(self.handle, arr), "fc_run_read_stats")
        raw = np.ctypeslib.as_array(arr)
        return {f: np.array(raw[f]) for f in STAT_FIELDS}

    def state(self) -> np.ndarray:
        out = np.zeros((self.n_chains, self.graph.n), dtype=np.int8)
        check(_lib.load().fc_run_read_state(self.handle, _p(out, ctypes.c_int8)), "fc_run_read_state")
        return out

    def pops(self) -> np.ndarray:
        out = np.zeros((self.n_chains, self.cfg.k), dtype=np.int64)
        check(_lib.load().fc_run_read_pops(self.handle, _p(out, ctypes.c_int64)), "fc_run_read_pops")
        return out

    def trace(self, chain: int = 0) -> np.ndarray:
        cap = self.cfg.trace_cap
        out = np.zeros(cap, dtype=RECORD_DTYPE)
        n = ctypes.c_int64(0)
        check(_lib.load().fc_run_read_trace(self.handle, chain, ctypes.cast(out.ctypes.data, _P(_lib.Record)),
                                            cap, ctypes.byref(n)), "fc_run_read_trace")
        if n.value > cap:
            raise OverflowError(f"trace capacity {cap} exceeded ({n.value} records)")
        return out[:n.value]

    def recom_trace(self, chain: int = 0) -> np.ndarray:
        """Per-proposal records of a traced ReCom chain (``fc_recom_record``)."""
        cap = self.cfg.trace_cap
        out = np.zeros(cap, dtype=RECOM_RECORD_DTYPE)
        n = ctypes.c_int64(0)
        check(_lib.load().fc_run_read_recom_trace(self.handle, chain,
                                                  ctypes.cast(out.ctypes.data, _P(_lib.RecomRecord)), cap,
                                                  ctypes.byref(n)), "fc_run_read_recom_trace")
        if n.value > cap:
            raise OverflowError(f"trace capacity {cap} exceeded ({n.value} records)")
        return out[:n.value]

    def trace_reset(self):
        check(_lib.load().fc_run_trace_reset(self.handle), "fc_run_trace_reset")

    def hist(self):
        E, n = self.graph.n_edges, self.graph.n
        ch = np.zeros((self.n_chains, E + 1), dtype=np.int64)
        nh = np.zeros((self.n_chains, self.nb_width()), dtype=np.int64)
        check(_lib.load().fc_run_read_hist(self.handle, _p(ch, ctypes.c_int64), _p(nh, ctypes.c_int64)))
        return ch, nh

    def cut_times(self) -> np.ndarray:
        out = np.zeros((self.n_chains, self.graph.n_edges), dtype=np.int64)
        check(_lib.load().fc_run_read_edges(self.handle, _p(out, ctypes.c_int64)))
        return out

    def flips(self):
        n = self.graph.n
        nf = np.zeros((self.n_chains, n), dtype=np.int64)
        ps = np.zeros((self.n_chains, n), dtype=np.int64)
        lf = np.zeros((self.n_chains, n), dtype=np.int64)
        check(_lib.load().fc_run_read_flips(self.handle, _p(nf, ctypes.c_int64), _p(ps, ctypes.c_int64),
                                            _p(lf, ctypes.c_int64)))
        return nf, ps, lf

    def flips_exact(self):
        """FC_DIAG_FLIPS_EXACT: (flip_count, occupancy, last_accept) [chains, n] -- the corrected
        companions of :meth:`flips` (include/flipchain.h)."""
        n = self.graph.n
        fc_ = np.zeros((self.n_chains, n), dtype=np.int64)
        occ = np.zeros((self.n_chains, n), dtype=np.int64)
        la = np.zeros((self.n_chains, n), dtype=np.int64)
        check(_lib.load().fc_run_read_flips_exact(self.handle, _p(fc_, ctypes.c_int64), _p(occ, ctypes.c_int64),
                                                  _p(la, ctypes.c_int64)))
        return fc_, occ, la

    def wait_expected(self) -> np.ndarray:
        """Rao-Blackwellised wait.txt companion (App. A.6 quirk 3): per chain, the sum over yields
        of E[geom_wait | |B|] = (N^k - 1)/|B| - 1 (:147-148), from the |B| histogram."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        check(_lib.load().fc_run_read_wait_expected(self.handle, _p(out, ctypes.c_double)))
        return out

    # ---- series diagnostics (FC_DIAG_SERIES) ------------------------------------------
    def events(self, chain: int = 0) -> np.ndarray:
        """Events of ``chain`` in the current series window (``fc_event``): the accepted flips of a
        flip run; of a ReCom run with a move log, one event per node an accepted step moved, the
        events of one step sharing their ``t``, ``cut`` and ``nb`` (a burst, ascending node id)."""
        cap = int(self.cfg.event_cap)
        out = np.zeros(cap, dtype=EVENT_DTYPE)
        n = ctypes.c_int64(0)
        check(_lib.load().fc_run_read_events(self.handle, chain, ctypes.cast(out.ctypes.data, _P(_lib.Event)),
                                             cap, ctypes.byref(n)), "fc_run_read_events")
        if n.value > cap:
            raise OverflowError(f"event capacity {cap} exceeded ({n.value} events)")
        return out[:n.value]

    def series_reset(self):
        check(_lib.load().fc_run_series_reset(self.handle), "fc_run_series_reset")

    def cut_series(self, chain: int = 0) -> np.ndarray:
        """|cut| at every yield of the window -- the reference's ``rce`` list
        (``grid_chain_sec11.py:367``) -- expanded on the host from the event log."""
        st = self.stats()
        t0, x0, T = int(st["series_t0"][chain]), int(st["series_cut0"][chain]), int(st["steps"][chain])
        ev = self.events(chain)
        bounds = np.concatenate([[t0], ev["t"], [T + 1]]).astype(np.int64)
        vals = np.concatenate([[x0], ev["cut"].astype(np.int64)])
        return np.repeat(vals, np.diff(bounds))

    def yield_values(self, field: str = "cut", chain: int = 0) -> np.ndarray:
        """Per-yield ``|cut|`` ("cut") or ``|B|`` ("nb") over the window: the reference's
        ``rce`` / ``rbn`` lists (``grid_chain_sec11.py:367,369``)."""
        st = self.stats()
        x0 = int(st["series_cut0" if field == "cut" else "series_nb0"][chain])
        ev = self.events(chain)
        return self.yield_series(np.concatenate([[x0], ev[field].astype(np.int64)]), chain)

    def autocorr(self, lags: Sequence[int]):
        """Device autocorrelation of the |cut| series over the window: ``(lag_sums, acf)``,
        each ``[n_chains, len(lags)]`` (``fc_run_autocorr``)."""
        lg = np.ascontiguousarray(lags, dtype=np.int32)
        sums = np.zeros((self.n_chains, lg.size), dtype=np.int64)
        acf = np.zeros((self.n_chains, lg.size), dtype=np.float64)
        check(_lib.load().fc_run_autocorr(self.handle, _p(lg, ctypes.c_int32), int(lg.size),
                                          _p(sums, ctypes.c_int64), _p(acf, ctypes.c_double)), "fc_run_autocorr")
        return sums, acf

    def autocorr_pairs(self, lags: Sequence[int]) -> np.ndarray:
        """``[n_chains, len(lags)]``: the (t, t + lag) pairs each lag's sum runs over in the
        current window, max(0, yields - lag) -- a lag at or beyond the window has none."""
        st = self.stats()
        n = (st["steps"] - st["series_t0"] + 1).astype(np.int64)
        return np.maximum(0, n[:, None] - np.asarray(lags, dtype=np.int64)[None, :])

    def frame_series(self, frame, chains: Optional[Sequence[int]] = None,
                     out: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """Slope / angle of the frame cut edges after every accepted flip of the window, on
        the device (``fc_run_frame_series``; ``grid_chain_sec11.py:55-78,371-394``).

        ``frame`` is a :class:`~flipcomplexityempirical_amd.graphs.SlopeFrame`.  Returns
        ``slope``, ``angle``, ``n_cut`` as ``[len(chains), max_events + 1]`` (entry 0: window
        start) and ``len`` per chain; use :meth:`yield_series` for the per-yield lists.
        ``out`` (optional): C-contiguous host buffers ``slope`` / ``angle`` (float64) and
        ``n_cut`` (int32) to fill instead of new arrays (a caller that reads many chunks keeps its
        pages mapped); the result then holds views of their leading ``nc * cap`` entries.  A
        buffer of another dtype or layout raises ``ValueError`` (the native call writes through
        raw pointers); buffers too small for this call's ``nc * cap`` entries are not used (fresh
        arrays are returned).  Entries past a chain's ``len`` are padding with undefined values."""
        ch = np.arange(self.n_chains) if chains is None else np.asarray(chains, dtype=np.int64)
        if ch.size == 0:
            raise ValueError("frame_series: no chains")
        c0, nc = int(ch.min()), int(ch.max() - ch.min() + 1)
        st = self.stats()
        cap = int(st["events"][c0:c0 + nc].max()) + 1
        # every entry is copied from the device (entries past a chain's ``len`` are padding)
        if out is not None:
            for key, dt in (("slope", np.float64), ("angle", np.float64), ("n_cut", np.int32)):
                buf = out.get(key)
                if not isinstance(buf, np.ndarray) or buf.dtype != dt or not buf.flags.c_contiguous \
                        or not buf.flags.writeable:
                    raise ValueError(f"frame_series: out[{key!r}] must be a writeable C-contiguous {np.dtype(dt)} array")
        if out is not None and min(out[key].size for key in ("slope", "angle", "n_cut")) >= nc * cap:
            # the buffers' leading nc * cap entries, viewed as [nc, cap]
            slope = out["slope"].reshape(-1)[:nc * cap].reshape(nc, cap)
            angle = out["angle"].reshape(-1)[:nc * cap].reshape(nc, cap)
            ncut = out["n_cut"].reshape(-1)[:nc * cap].reshape(nc, cap)
        else:
            slope = np.empty((nc, cap), dtype=np.float64)
            angle = np.empty((nc, cap), dtype=np.float64)
            ncut = np.empty((nc, cap), dtype=np.int32)
        ln = np.zeros(nc, dtype=np.int64)
        eu = np.ascontiguousarray(frame.eu, dtype=np.int32)
        ev = np.ascontiguousarray(frame.ev, dtype=np.int32)
        mid = np.ascontiguousarray(frame.mid, dtype=np.float64)
        check(_lib.load().fc_run_frame_series(self.handle, c0, nc, int(eu.size), _p(eu, ctypes.c_int32),
                                              _p(ev, ctypes.c_int32), _p(mid, ctypes.c_double),
                                              float(frame.center[0]), float(frame.center[1]), cap,
                                              _p(slope, ctypes.c_double), _p(angle, ctypes.c_double),
                                              _p(ncut, ctypes.c_int32), _p(ln, ctypes.c_int64)),
              "fc_run_frame_series")
        sel = ch - c0
        if sel.size == nc and np.array_equal(sel, np.arange(nc)):  # a contiguous range: no copies
            return {"slope": slope, "angle": angle, "n_cut": ncut, "len": ln}
        return {"slope": slope[sel], "angle": angle[sel], "n_cut": ncut[sel], "len": ln[sel]}

    def frame_series_changes(self, frame, c0: int = 0, nc: Optional[int] = None,
                             out: Optional[Dict[str, np.ndarray]] = None, query: bool = False) -> Dict[str, np.ndarray]:
        """Change points of the slope / angle series of chains ``c0 .. c0 + nc - 1``
        (``fc_run_frame_series_changes``): ``offsets`` [nc + 1] and flat ``t`` (int64), ``slope``,
        ``angle`` (float64); chain ``c0 + i`` owns entries ``offsets[i]:offsets[i + 1]``, each
        value holding from its ``t`` to the next entry's -- what the reference's slope / angle
        plots draw (``grid_chain_sec11.py:476-484``); :meth:`changes_to_yields` expands one chain
        to its per-yield lists (``:382,394``).  ``out`` (optional): C-contiguous int64 / float64 /
        float64 buffers ``t`` / ``slope`` / ``angle`` to fill (e.g. pinned with
        :func:`pin_host`); used when large enough, the result then holds views of them.
        ``query``: only the offsets (sizing buffers)."""
        nc = self.n_chains - c0 if nc is None else int(nc)
        L = _lib.load()
        eu = np.ascontiguousarray(frame.eu, dtype=np.int32)
        ev = np.ascontiguousarray(frame.ev, dtype=np.int32)
        mid = np.ascontiguousarray(frame.mid, dtype=np.float64)
        off = np.zeros(nc + 1, dtype=np.int64)
        args = (self.handle, int(c0), nc, int(eu.size), _p(eu, ctypes.c_int32), _p(ev, ctypes.c_int32),
                _p(mid, ctypes.c_double), float(frame.center[0]), float(frame.center[1]))
        if out is not None and not query:
            for key, dt in (("t", np.int64), ("slope", np.float64), ("angle", np.float64)):
                b = out.get(key)
                if not isinstance(b, np.ndarray) or b.dtype != dt or not b.flags.c_contiguous or not b.flags.writeable:
                    raise ValueError(f"frame_series_changes: out[{key!r}] must be a writeable C-contiguous "
                                     f"{np.dtype(dt)} array")
            # one call: count, offsets, write and copy into the caller's buffers when they hold
            # every change point (the offsets come back either way)
            cap = min(out[key].size for key in ("t", "slope", "angle"))
            flat = {key: out[key].reshape(-1) for key in ("t", "slope", "angle")}
            rc = L.fc_run_frame_series_changes(*args, cap, _p(off, ctypes.c_int64), _p(flat["t"], ctypes.c_int64),
                                               _p(flat["slope"], ctypes.c_double), _p(flat["angle"], ctypes.c_double))
            total = int(off[-1])
            if rc == 0:
                return {"offsets": off, **{key: b[:total] for key, b in flat.items()}}
            if total <= cap:
                check(rc, "fc_run_frame_series_changes")
        else:
            check(L.fc_run_frame_series_changes(*args, 0, _p(off, ctypes.c_int64), _P(ctypes.c_int64)(),
                                                _P(ctypes.c_double)(), _P(ctypes.c_double)()),
                  "fc_run_frame_series_changes")
            total = int(off[-1])
            if query:
                return {"offsets": off}
        bufs = {"t": np.empty(total, dtype=np.int64), "slope": np.empty(total), "angle": np.empty(total)}
        check(L.fc_run_frame_series_changes(*args, total, _p(off, ctypes.c_int64), _p(bufs["t"], ctypes.c_int64),
                                            _p(bufs["slope"], ctypes.c_double), _p(bufs["angle"], ctypes.c_double)),
              "fc_run_frame_series_changes")
        return {"offsets": off, **bufs}

    def changes_to_yields(self, ch: Dict[str, np.ndarray], i: int, chain: int, key: str = "slope") -> np.ndarray:
        """Per-yield list (the reference's ``slopes`` / ``angles``, :382,394) of ``chain`` from
        entry ``i`` of a :meth:`frame_series_changes` result."""
        lo, hi = int(ch["offsets"][i]), int(ch["offsets"][i + 1])
        T = int(self.stats()["steps"][chain])
        bounds = np.concatenate([ch["t"][lo:hi], [T + 1]]).astype(np.int64)
        return np.repeat(ch[key][lo:hi], np.diff(bounds))

    def yield_series(self, values: np.ndarray, chain: int = 0) -> np.ndarray:
        """Expand a per-event series (entry 0 = window start, as ``frame_series`` returns it)
        to one value per yield of the window, as the reference's ``slopes`` / ``angles``
        lists hold them (``grid_chain_sec11.py:382,394``)."""
        st = self.stats()
        t0, T = int(st["series_t0"][chain]), int(st["steps"][chain])
        ev = self.events(chain)
        bounds = np.concatenate([[t0], ev["t"], [T + 1]]).astype(np.int64)
        return np.repeat(np.asarray(values)[:ev.size + 1], np.diff(bounds))

    def _int64_series(self, entry: str, c0: int, nc: Optional[int], rows: Dict[str, Optional[tuple]]):
        """Call the series entry point ``entry(handle, c0, nc, *outputs)``: ``rows`` gives, in the
        entry point's order, each int64 output's shape per chain (None: not asked for, a null
        pointer).  Returns the zero-filled ``[nc, *shape]`` outputs and ``yields``."""
        nc = self.n_chains - c0 if nc is None else int(nc)
        out = {key: np.zeros((max(nc, 0),) + shape, dtype=np.int64) for key, shape in rows.items()
               if shape is not None}
        check(getattr(_lib.load(), entry)(self.handle, int(c0), nc, *(_p(out.get(key), ctypes.c_int64) for key in rows)),
              entry)
        st = self.stats()
        out["yields"] = (st["steps"] - st["series_t0"] + 1)[c0:c0 + nc].astype(np.int64)
        return out

    # ---- election series ----------------------------------------------
    def set_elections(self, columns, elections: Sequence = (), gap_edges=None) -> "FlipRun":
        """Attach node vote columns (``fc_run_set_elections``): ``columns`` is ``[n, n_cols]``
        non-negative integers in canonical node order, ``elections`` a list of ``(col_a, col_b)``
        column pairs (at most 4; none keeps the tallies only), ``gap_edges`` the strictly ascending
        int64 bin edges of the efficiency-gap histogram in its doubled integer units (at most 256;
        None: no histogram).  Callable again to replace them; a restored run needs it again."""
        cols = np.asarray(columns)
        if cols.ndim == 1:
            cols = cols[:, None]
        if cols.ndim != 2 or cols.shape[0] != self.graph.n:
            raise ValueError("columns must be [n, n_cols]")
        if not np.issubdtype(cols.dtype, np.integer):
            raise ValueError("columns must be integers")
        if cols.size and (cols.min() < -2 ** 31 or cols.max() > 2 ** 31 - 1):
            raise ValueError("columns must hold int32 values")  # (the library checks the rest)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        el = np.ascontiguousarray(np.asarray(list(elections), dtype=np.int32).reshape(-1, 2))
        ca, cb = np.ascontiguousarray(el[:, 0]), np.ascontiguousarray(el[:, 1])
        edges = np.ascontiguousarray([] if gap_edges is None else gap_edges, dtype=np.int64).reshape(-1)
        check(_lib.load().fc_run_set_elections(self.handle, int(cols.shape[1]), _p(cols, ctypes.c_int32),
                                               int(el.shape[0]), _p(ca, ctypes.c_int32), _p(cb, ctypes.c_int32),
                                               int(edges.size), _p(edges, ctypes.c_int64)), "fc_run_set_elections")
        self._elections = (int(cols.shape[1]), int(el.shape[0]), int(edges.size))
        return self

    def election_series(self, c0: int = 0, nc: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Election statistics of chains ``c0 .. c0 + nc - 1`` over the series window, replayed
        on the device from the event log (``fc_run_election_series``; include/flipchain.h):
        ``tally_now`` / ``tally_sum`` ``[nc, k, n_cols]``, ``seats_hist`` ``[nc, n_el, k + 1]``,
        ``wins_sum`` ``[nc, n_el, k]``, ``gap_sum`` ``[nc, n_el]``, ``gap_hist``
        ``[nc, n_el, n_edges + 1]`` (only with ``gap_edges``) and ``yields`` ``[nc]``, the yields of
        each chain's window.  All int64."""
        n_cols, n_el, n_edges = getattr(self, "_elections", (1, 0, 0))
        k = self.cfg.k
        return self._int64_series("fc_run_election_series", c0, nc, {
            "tally_now": (k, n_cols), "tally_sum": (k, n_cols), "seats_hist": (n_el, k + 1), "wins_sum": (n_el, k),
            "gap_sum": (n_el,), "gap_hist": (n_el, n_edges + 1) if n_edges else None})

    # ---- compactness series -------------------------------------------
    def set_shapes(self, area, edge_len, exterior=None, pp_edges=None) -> "FlipRun":
        """Attach the units' geometry (``fc_run_set_shapes``): ``area`` ``[n]`` and ``exterior``
        ``[n]`` (the length of a unit's boundary on the outside of the whole region; None: 0) in
        canonical node order, ``edge_len`` ``[E]`` (the length two adjacent units share) in
        canonical edge order, all non-negative int32; ``pp_edges`` the strictly ascending int64 bin
        edges of the Polsby-Popper histograms in units of ``Q = floor(2**20 A / P**2)`` (at most
        64; None: no histograms).  Callable again to replace them; a restored run needs it again."""
        def vec(x, size, what):
            x = np.asarray(x)
            if x.shape != (size,) or not np.issubdtype(x.dtype, np.integer):
                raise ValueError(f"{what} must be {size} integers")
            if x.size and (x.min() < -2 ** 31 or x.max() > 2 ** 31 - 1):
                raise ValueError(f"{what} must hold int32 values")  # (the library checks the rest)
            return np.ascontiguousarray(x, dtype=np.int32)
        ar = vec(area, self.graph.n, "area")
        el = vec(edge_len, self.graph.n_edges, "edge_len")
        ex = None if exterior is None else vec(exterior, self.graph.n, "exterior")
        edges = np.ascontiguousarray([] if pp_edges is None else pp_edges, dtype=np.int64).reshape(-1)
        check(_lib.load().fc_run_set_shapes(self.handle, _p(ar, ctypes.c_int32), _p(ex, ctypes.c_int32),
                                            _p(el, ctypes.c_int32), int(edges.size), _p(edges, ctypes.c_int64)),
              "fc_run_set_shapes")
        self._shape_edges = int(edges.size)
        return self

    def shape_series(self, c0: int = 0, nc: Optional[int] = None) -> Dict[str, np.ndarray]:
        """District shapes of chains ``c0 .. c0 + nc - 1`` over the series window, replayed on the
        device from the event log (``fc_run_shape_series``; include/flipchain.h): ``area_now`` /
        ``perim_now`` / ``perim_sum`` / ``pp_now`` / ``pp_sum`` ``[nc, k]``, ``pp_min_sum`` ``[nc]``,
        ``pp_hist`` ``[nc, k, n_edges + 1]`` and ``pp_min_hist`` ``[nc, n_edges + 1]`` (only with
        ``pp_edges``) and ``yields`` ``[nc]``, the yields of each chain's window.  All int64; the
        Polsby-Popper score of a ``pp`` value ``Q`` is ``4 pi Q / 2**20``."""
        n_edges = getattr(self, "_shape_edges", 0)
        k = self.cfg.k
        return self._int64_series("fc_run_shape_series", c0, nc, {
            "area_now": (k,), "perim_now": (k,), "perim_sum": (k,), "pp_now": (k,), "pp_sum": (k,), "pp_min_sum": (),
            "pp_hist": (k, n_edges + 1) if n_edges else None, "pp_min_hist": (n_edges + 1,) if n_edges else None})

    # ---- locality-splits series ---------------------------------------
    def set_localities(self, node_loc) -> "FlipRun":
        """Attach a node labelling (``fc_run_set_localities``): ``node_loc`` ``[n]`` integer labels
        ``0 .. n_loc - 1`` in canonical node order (counties, municipalities), every label used.
        Callable again to replace it; a restored run needs it again."""
        loc = np.asarray(node_loc)
        if loc.shape != (self.graph.n,) or not np.issubdtype(loc.dtype, np.integer):
            raise ValueError(f"node_loc must be {self.graph.n} integers")
        if loc.size and (loc.min() < -2 ** 31 or loc.max() > 2 ** 31 - 2):
            raise ValueError("node_loc must hold int32 labels")  # (the library checks the rest)
        loc = np.ascontiguousarray(loc, dtype=np.int32)
        n_loc = int(loc.max()) + 1 if loc.size else 0
        check(_lib.load().fc_run_set_localities(self.handle, n_loc, _p(loc, ctypes.c_int32)), "fc_run_set_localities")
        sizes = np.bincount(loc, minlength=n_loc)
        self._localities = (n_loc, int(np.minimum(sizes, self.cfg.k).sum()) - n_loc)
        return self

    def split_series(self, c0: int = 0, nc: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Locality splits of chains ``c0 .. c0 + nc - 1`` over the series window, replayed on the
        device from the event log (``fc_run_split_series``; include/flipchain.h): ``cells_now``
        ``[nc, n_loc, k]``, ``split_sum`` / ``parts_sum`` ``[nc, n_loc]``, ``dlocs_sum`` ``[nc, k]``,
        ``sq_sum`` ``[nc]``, ``splits_hist`` ``[nc, n_loc + 1]``, ``excess_hist`` ``[nc, X + 1]``
        (``X = min(x_max, 1023)``) and ``yields`` ``[nc]``, all int64; and, derived from ``cells_now``
        on the host, ``parts_now`` ``[nc, n_loc]``, ``splits_now`` / ``excess_now`` / ``sq_now``
        ``[nc]``, ``dlocs_now`` ``[nc, k]``, with ``x_max`` (an int) the largest possible excess."""
        n_loc, x_max = getattr(self, "_localities", (1, 0))
        k = self.cfg.k
        out = self._int64_series("fc_run_split_series", c0, nc, {
            "cells_now": (n_loc, k), "split_sum": (n_loc,), "parts_sum": (n_loc,), "dlocs_sum": (k,), "sq_sum": (),
            "splits_hist": (n_loc + 1,), "excess_hist": (min(x_max, 1023) + 1,)})
        occ = out["cells_now"] > 0
        out["parts_now"] = occ.sum(axis=2).astype(np.int64)
        out["splits_now"] = (out["parts_now"] >= 2).sum(axis=1).astype(np.int64)
        out["excess_now"] = (out["parts_now"] - 1).sum(axis=1).astype(np.int64)
        out["sq_now"] = (out["cells_now"] ** 2).sum(axis=(1, 2)).astype(np.int64)
        out["dlocs_now"] = occ.sum(axis=1).astype(np.int64)
        out["x_max"] = x_max
        return out

    # ---- plan samples -------------------------------------------------
    def sample_plans(self, times=None, every: Optional[int] = None, c0: int = 0, nc: Optional[int] = None,
                     plans: bool = True, pops: bool = True) -> Dict[str, np.ndarray]:
        """The plans chains ``c0 .. c0 + nc - 1`` hold at the yields ``times`` (absolute yield
        indices inside the series window, strictly increasing, the same for every chain), replayed
        on the device from the event log (``fc_run_sample_plans``; include/flipchain.h).  ``every``
        instead of ``times`` samples the run's own window: ``series_t0, + every, ... <= steps``.
        Returns ``times`` ``[m]``, ``plans`` int8 ``[nc, m, n]`` (district indices as
        :meth:`state` reports them; left out with ``plans=False``), ``cut`` / ``nb`` / ``dist0``
        int64 ``[nc, m]`` (|cut|, |B| and the Hamming distance to the window-start plan), ``pops``
        int64 ``[nc, m, k]`` (left out with ``pops=False``) and ``yields`` ``[nc]``, the yields of
        each chain's window."""
        nc = self.n_chains - c0 if nc is None else int(nc)
        if (times is None) == (every is None):
            raise ValueError("give either times or every")
        st = None
        if times is None:
            st = self.stats()
            sel = slice(max(int(c0), 0), max(int(c0), 0) + max(nc, 0))
            t0, steps = st["series_t0"][sel], st["steps"][sel]
            tm = sample_times(int(t0.max()), int(steps.min()), every) if t0.size else np.zeros(0, dtype=np.int64)
        else:
            tm = np.asarray(times)
            if tm.ndim != 1:
                raise ValueError("times must be one-dimensional")
            if tm.size and not np.issubdtype(tm.dtype, np.integer):
                raise ValueError("times must be integers")
            tm = np.ascontiguousarray(tm, dtype=np.int64)
            if tm.size > 1 and (np.diff(tm) <= 0).any():
                raise ValueError("times must be strictly increasing")
        m, n, k = int(tm.size), self.graph.n, self.cfg.k
        rows = max(nc, 0)
        out = {"times": tm, "cut": np.zeros((rows, m), dtype=np.int64), "nb": np.zeros((rows, m), dtype=np.int64),
               "dist0": np.zeros((rows, m), dtype=np.int64)}
        if plans:
            out["plans"] = np.zeros((rows, m, n), dtype=np.int8)
        if pops:
            out["pops"] = np.zeros((rows, m, k), dtype=np.int64)
        check(_lib.load().fc_run_sample_plans(self.handle, int(c0), nc, m, _p(tm, ctypes.c_int64),
                                              _p(out.get("plans"), ctypes.c_int8), _p(out["cut"], ctypes.c_int64),
                                              _p(out["nb"], ctypes.c_int64), _p(out["dist0"], ctypes.c_int64),
                                              _p(out.get("pops"), ctypes.c_int64)), "fc_run_sample_plans")
        st = self.stats() if st is None else st
        out["yields"] = (st["steps"] - st["series_t0"] + 1)[c0:c0 + nc].astype(np.int64)
        return out

    def sample_plans_ms(self):
        """Device ms of the last :meth:`sample_plans` call's kernel and of its copy of the plan rows
        to the host (``fc_run_sample_plans_ms``; HIP events on the run's stream)."""
        k_ms, c_ms = ctypes.c_float(0), ctypes.c_float(0)
        check(_lib.load().fc_run_sample_plans_ms(self.handle, ctypes.byref(k_ms), ctypes.byref(c_ms)),
              "fc_run_sample_plans_ms")
        return float(k_ms.value), float(c_ms.value)

    # ---- heat-map series ----------------------------------------------
    HEAT_OUTPUTS = ("cut_hist", "nb_hist", "cut_times", "moves", "last_move", "dwell")

    def heat_series(self, c0: int = 0, nc: Optional[int] = None, want: Sequence[str] = HEAT_OUTPUTS,
                    lds_rows: bool = False) -> Dict[str, np.ndarray]:
        """The heat maps of chains ``c0 .. c0 + nc - 1`` over the series window, replayed on the
        device from the event log (``fc_run_heat_series``; include/flipchain.h): ``cut_hist``
        ``[nc, E + 1]`` and ``nb_hist`` ``[nc, nb_width]`` (yields per |cut| and |B|), ``cut_times``
        ``[nc, E]`` (yields each canonical edge is cut), ``moves`` / ``last_move`` ``[nc, n]``
        (logged events on each node and the yield of the last), ``dwell`` ``[nc, n, k]`` (yields each
        node spends in each district) and ``yields`` ``[nc]``, all int64.  ``want`` names the
        outputs to compute (the others are left out).  The replay accumulates in the output rows in
        device memory; ``lds_rows`` keeps a chain's arrays in LDS instead when they fit (same
        output, slower as measured; :meth:`heat_series_info` tells which form ran).  Flip runs of
        any k and ReCom runs with a move log."""
        unknown = [key for key in want if key not in self.HEAT_OUTPUTS]
        if unknown:
            raise ValueError(f"heat_series: unknown outputs {unknown} (known: {', '.join(self.HEAT_OUTPUTS)})")
        n, k = self.graph.n, self.cfg.k
        shapes = {"cut_hist": (self.graph.n_edges + 1,), "nb_hist": (self.nb_width(),),
                  "cut_times": (self.graph.n_edges,), "moves": (n,), "last_move": (n,), "dwell": (n, k)}
        nc = self.n_chains - c0 if nc is None else int(nc)
        out = {key: np.zeros((max(nc, 0),) + shapes[key], dtype=np.int64) for key in self.HEAT_OUTPUTS if key in want}
        check(_lib.load().fc_run_heat_series(self.handle, int(c0), nc, _lib.FC_HEAT_LDS_ROWS if lds_rows else 0,
                                             *(_p(out.get(key), ctypes.c_int64) for key in self.HEAT_OUTPUTS)),
              "fc_run_heat_series")
        st = self.stats()
        out["yields"] = (st["steps"] - st["series_t0"] + 1)[c0:c0 + nc].astype(np.int64)
        return out

    def heat_series_info(self) -> Dict[str, Any]:
        """The last :meth:`heat_series` call that launched (``fc_run_heat_series_info``): ``form``
        ("lds" or "global_rows"), ``lds_bytes`` of one workgroup and the kernel's device ``ms``."""
        form, lds, ms = ctypes.c_int32(-1), ctypes.c_int64(0), ctypes.c_float(0)
        check(_lib.load().fc_run_heat_series_info(self.handle, ctypes.byref(form), ctypes.byref(lds), ctypes.byref(ms)),
              "fc_run_heat_series_info")
        return {"form": "lds" if form.value == 0 else "global_rows", "lds_bytes": int(lds.value), "ms": float(ms.value)}

    # ---- short bursts --------------------------------------------------
    BURST_OUTPUTS = ("best_score", "best_t", "start_score", "end_score", "best_cut", "best_nb")

    def burst_select(self, metric: "BurstMetric", rewind: bool = False, c0: int = 0, nc: Optional[int] = None,
                     plans: bool = False) -> Dict[str, np.ndarray]:
        """Scores every yield of the series window of chains ``c0 .. c0 + nc - 1`` by ``metric`` on
        the device (``fc_run_burst_select``; include/flipchain.h): ``best_score`` and ``best_t`` (the
        latest yield with the best score), ``start_score`` / ``end_score`` (at ``series_t0`` and at
        ``steps``), ``best_cut`` / ``best_nb`` (|cut| and |B| at ``best_t``), int64 ``[nc]`` each, and
        with ``plans`` ``best_plan`` int8 ``[nc, n]``, the assignment at ``best_t``.  ``rewind``
        (ReCom runs only) restarts every chain of the range from its best plan: its state, cut / nb
        and a fresh series window there; the draw counter, ``steps`` and the sums continue.  The vote
        kinds read the columns of :meth:`set_elections`."""
        nc = self.n_chains - c0 if nc is None else int(nc)
        rows = max(nc, 0)
        out = {key: np.zeros(rows, dtype=np.int64) for key in self.BURST_OUTPUTS}
        if plans:
            out["best_plan"] = np.zeros((rows, self.graph.n), dtype=np.int8)
        m = metric.struct()
        check(_lib.load().fc_run_burst_select(self.handle, int(c0), nc, ctypes.byref(m),
                                              _lib.FC_BURST_REWIND if rewind else 0,
                                              *(_p(out[key], ctypes.c_int64) for key in self.BURST_OUTPUTS),
                                              _p(out.get("best_plan"), ctypes.c_int8)), "fc_run_burst_select")
        return out

    def burst_select_ms(self) -> float:
        """Device ms of the last :meth:`burst_select` call's kernel (``fc_run_burst_select_ms``)."""
        ms = ctypes.c_float(0)
        check(_lib.load().fc_run_burst_select_ms(self.handle, ctypes.byref(ms)), "fc_run_burst_select_ms")
        return float(ms.value)

    # ---- replica exchange (DESIGN.md "Replica exchange") ------------------------------
    def set_ladders(self, ladders: Sequence[Sequence[int]], hist: bool = False) -> "FlipRun":
        """``ladders``: lists of local chain indices, rung 0 first (``fc_run_set_ladders``; once
        per run).  ``hist``: keep the |cut| / |B| histograms per rung too (needs FC_DIAG_HIST)."""
        lad = [np.asarray(x, dtype=np.int32).reshape(-1) for x in ladders]
        off = np.zeros(len(lad) + 1, dtype=np.int32)
        off[1:] = np.cumsum([x.size for x in lad])
        mem = np.ascontiguousarray(np.concatenate(lad) if lad else np.zeros(0, dtype=np.int32), dtype=np.int32)
        check(_lib.load().fc_run_set_ladders(self.handle, len(lad), _p(off, ctypes.c_int32), _p(mem, ctypes.c_int32),
                                             _lib.FC_LADDER_HIST if hist else 0), "fc_run_set_ladders")
        self._ladder_off, self._ladder_hist = off, bool(hist)
        return self

    def exchange(self, parity: int = -1, stream: Optional[int] = None) -> "FlipRun":
        """One exchange round between the ``steps`` launches it separates (asynchronous);
        ``parity`` -1: the round counter's."""
        check(_lib.load().fc_run_exchange(self.handle, int(parity), ctypes.c_void_p(stream) if stream else None),
              "fc_run_exchange")
        return self

    def rungs(self):
        """``(rung_of [n_chains], chain_at)``: the rung each chain holds (-1: no ladder) and, per
        ladder, the chain at each rung."""
        off = getattr(self, "_ladder_off", np.zeros(1, dtype=np.int32))
        rung_of = np.zeros(self.n_chains, dtype=np.int32)
        flat = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
        check(_lib.load().fc_run_read_rungs(self.handle, _p(rung_of, ctypes.c_int32), _p(flat, ctypes.c_int32)),
              "fc_run_read_rungs")
        return rung_of, [flat[off[i]:off[i + 1]].copy() for i in range(off.size - 1)]

    def bases_now(self) -> np.ndarray:
        """The base every chain runs at now (``fc_run_read_bases``)."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        check(_lib.load().fc_run_read_bases(self.handle, _p(out, ctypes.c_double)), "fc_run_read_bases")
        return out

    def rung_stats(self) -> Dict[str, np.ndarray]:
        """Per-slot statistics (slot = ladder offset + rung, in ``set_ladders`` order): the
        ``fc_rung_stats`` fields as int64 arrays, ``ladder_off``, and with ``hist`` the per-slot
        ``cut_hist`` / ``nb_hist`` (``fc_run_read_rung_stats``)."""
        off = getattr(self, "_ladder_off", np.zeros(1, dtype=np.int32))
        M = int(off[-1])
        arr = (_lib.RungStats * max(M, 1))()
        ch = nh = None
        if getattr(self, "_ladder_hist", False):
            ch = np.zeros((M, self.graph.n_edges + 1), dtype=np.int64)
            nh = np.zeros((M, self.nb_width()), dtype=np.int64)
        check(_lib.load().fc_run_read_rung_stats(self.handle, arr, _p(ch, ctypes.c_int64), _p(nh, ctypes.c_int64)),
              "fc_run_read_rung_stats")
        raw = np.ctypeslib.as_array(arr)[:M]
        out = {f: np.array(raw[f]) for f, _ in _lib.RungStats._fields_}
        out["ladder_off"] = off.copy()
        if ch is not None:
            out["cut_hist"], out["nb_hist"] = ch, nh
        return out

    def diag_paths(self) -> Dict[str, int]:
        """The paths the memory-dependent diagnostics took (``fc_run_diag_paths``): tally-log
        entries per chain granted / asked for, and whether the last change-point call was staged."""
        cap, want, staged = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        check(_lib.load().fc_run_diag_paths(self.handle, ctypes.byref(cap), ctypes.byref(want), ctypes.byref(staged)),
              "fc_run_diag_paths")
        return {"tally_log_cap": int(cap.value), "tally_log_wanted": int(want.value),
                "series_staged": int(staged.value)}

    def tally_plan(self) -> Dict[str, object]:
        """The pass plan of the last k = 2 tally reduce (``fc_run_tally_plan``): the LDS limit it
        was planned for, ``passes`` as (LDS array mask, LDS bytes) pairs and the mask of the arrays
        under global atomics.  No pass: no reduce has run."""
        limit, n, g = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_uint32(0)
        masks, nbytes = (ctypes.c_uint32 * 9)(), (ctypes.c_int64 * 9)()
        check(_lib.load().fc_run_tally_plan(self.handle, ctypes.byref(limit), ctypes.byref(n), masks, nbytes, 9,
                                            ctypes.byref(g)), "fc_run_tally_plan")
        return {"limit": int(limit.value), "passes": [(int(masks[i]), int(nbytes[i])) for i in range(n.value)],
                "global_mask": int(g.value)}

    def ring_table(self) -> Dict[str, int]:
        """The k = 2 ring-verdict table (``fc_run_ring_table``): the classes the graph's rings fall
        into and whether the run holds a table (1: its lean node-stream launches read it) or none (0)."""
        classes, used = ctypes.c_int32(0), ctypes.c_int32(0)
        check(_lib.load().fc_run_ring_table(self.handle, ctypes.byref(classes), ctypes.byref(used)), "fc_run_ring_table")
        return {"classes": int(classes.value), "in_use": int(used.value)}

    def nb_width(self) -> int:
        """Entries of a chain's |B| histogram row (``fc_run_nb_width``): n + 1, or the largest
        pair count + 1 with ``FC_FLAG_NB_PAIRS``."""
        return int(_lib.load().fc_run_nb_width(self.handle))

    def chain_lds_bytes(self) -> int:
        """LDS bytes of one chain's device state (``fc_run_chain_lds_bytes``)."""
        return int(_lib.load().fc_run_chain_lds_bytes(self.handle))

    def kernel_name(self) -> str:
        """The flip-kernel instance the last ``steps`` call launched (rocprofv3 spelling)."""
        buf = ctypes.create_string_buffer(128)
        check(_lib.load().fc_run_kernel_name(self.handle, buf, 128), "fc_run_kernel_name")
        return buf.value.decode()

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().fc_run_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
