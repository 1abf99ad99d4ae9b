"""Cost of the heat-map series: python tools/heat_series_cost.py [chains] [repeats]

Two windows on sec11 (40x40, k = 2), all chains in one call, the two accumulation forms
alternating, `repeats` calls each after one warm-up call per form:
  c2     the bench's C2 shape with its full diagnostics and the event log (bases[g % 10], alignment
         (g // 10) % 3, seed 0x5EED0002), one launch of 100,000 steps; every output but dwell;
  recom  the ReCom window of DESIGN.md §5g (tree proposal, always_accept, 20 steps per launch,
         event_cap = 20 n); every output.
Prints one JSON line per window: the launch that made the window (fc_run_last_ms), the events per
chain, and per form the kernel's HIP-event ms (median, min, max), its LDS bytes per workgroup and
the host wall clock around the synchronous call.  Measurements only: no pass / fail threshold."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
spec = G.sec11_graph()
plans = [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]
_, (lo, hi) = G.population_bounds(spec.n, 2, 0.1)
graph = FlipGraph(spec)


def measure(run, want):
    forms = {}
    for g in (False, True):  # warm-up: grows the run's buffers, uploads the rows
        run.heat_series(want=want, lds_rows=g)
    for _ in range(REP):
        for g in (False, True):
            t0 = time.perf_counter()
            run.heat_series(want=want, lds_rows=g)
            wall = (time.perf_counter() - t0) * 1e3
            info = run.heat_series_info()
            f = forms.setdefault(info["form"], {"kernel_ms": [], "wall_ms": [], "lds_bytes": info["lds_bytes"]})
            f["kernel_ms"].append(info["ms"])
            f["wall_ms"].append(wall)
    return {name: {"lds_bytes": f["lds_bytes"],
                   "kernel_ms": {"median": float(np.median(f["kernel_ms"])), "min": min(f["kernel_ms"]),
                                 "max": max(f["kernel_ms"])},
                   "wall_ms_median": float(np.median(f["wall_ms"]))} for name, f in forms.items()}


# C2: flip run, full diagnostics, one 100,000-step window
steps = 100000
inits = np.stack([plans[(c // 10) % 3] for c in range(C)])
bases = np.asarray([G.SEC11_BASES[c % 10] for c in range(C)])
full = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_FLIPS | _lib.FC_DIAG_SERIES
run = FlipRun(graph, inits, RunConfig(seed=0x5EED0002, pop_lo=lo, pop_hi=hi, diag_mask=full, event_cap=steps + 1),
              bases=bases)
run.steps(steps)
run.sync()
launch_ms = run.last_ms()
ev = run.stats()["events"]
want = ("cut_hist", "nb_hist", "cut_times", "moves", "last_move")
out = {"window": "c2", "shape": f"sec11 k=2, {C} chains, one launch of {steps} steps, outputs {'/'.join(want)}",
       "launch_ms": launch_ms, "events_per_chain": {"mean": float(ev.mean()), "min": int(ev.min()), "max": int(ev.max())},
       "repeats": REP, "forms": measure(run, want)}
ch, _ = run.hist()
assert np.array_equal(run.heat_series(want=("cut_hist",))["cut_hist"], ch)
run.close()
print(json.dumps(out), flush=True)

# ReCom: 20 steps per window
S = 20
inits = np.stack([plans[c % 3] for c in range(C)])
cfg = RunConfig(proposal=_lib.FC_PROPOSE_RECOM, seed=0x5EED0010, pop_lo=lo, pop_hi=hi, base=1.0,
                recom_pop_target=spec.n / 2, recom_epsilon=0.05, recom_node_repeats=1,
                diag_mask=_lib.FC_DIAG_SERIES, event_cap=S * spec.n)
run = FlipRun(graph, inits, cfg)
run.steps(S)  # warm-up launch
run.series_reset()
run.steps(S)
run.sync()
launch_ms = run.last_ms()
ev = run.stats()["events"]
out = {"window": "recom", "shape": f"sec11 k=2 ReCom, {C} chains x {S} steps, every output",
       "launch_ms": launch_ms, "events_per_chain": {"mean": float(ev.mean()), "min": int(ev.min()), "max": int(ev.max())},
       "repeats": REP, "forms": measure(run, FlipRun.HEAT_OUTPUTS)}
run.close()
print(json.dumps(out), flush=True)
