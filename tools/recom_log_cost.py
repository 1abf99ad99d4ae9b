"""Cost of the ReCom move log (DESIGN.md "ReCom move log"): python tools/recom_log_cost.py [chains] [steps/launch] [launches]

The bench's ReCom shape: sec11 40x40, k=2, the reference's tree_proposal parameters, population
bound 0.1, always_accept, 4096 chains x 20 steps per launch.  Prints one JSON line:
  kernel_ms_off / kernel_ms_on   HIP-event time per launch (fc_run_last_ms) of the lean instance and
                                 of the logging one (event_cap = steps x n, a window per launch);
  moved_per_accepted_step        events / accepted steps over the logged launches;
  series_ms                      host wall clock around each of the five series calls over one
                                 launch's window, all chains (each call downloads the scalars, runs
                                 its kernels and copies its outputs, then synchronises);
                                 sample_plans also with its kernel's HIP-event time.
Measurements only: there is no pass / fail threshold."""
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
S = int(sys.argv[2]) if len(sys.argv) > 2 else 20
IT = int(sys.argv[3]) if len(sys.argv) > 3 else 10
spec = G.sec11_graph()
plans = [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]
inits = np.stack([plans[c % 3] for c in range(C)])
_, (lo, hi) = G.population_bounds(spec.n, 2, 0.1)
graph = FlipGraph(spec)


def make(log):
    cfg = RunConfig(proposal=_lib.FC_PROPOSE_RECOM, seed=0x5EED0010, pop_lo=lo, pop_hi=hi, base=1.0,
                    recom_pop_target=spec.n / 2, recom_epsilon=0.05, recom_node_repeats=1,
                    diag_mask=_lib.FC_DIAG_SERIES if log else 0, event_cap=S * spec.n if log else 0)
    return FlipRun(graph, inits, cfg)


def launches(run, log):
    """IT timed launches after a warm-up one; a logged run starts a new window before each."""
    ms, events, accepted = [], 0, 0
    for i in range(IT + 1):
        if log:
            run.series_reset()
        a0 = run.stats()["accepted"].sum()
        run.steps(S)
        run.sync()
        if i:
            ms.append(float(run.timings()[-1]))
            st = run.stats()
            events += int(st["events"].sum())
            accepted += int(st["accepted"].sum() - a0)
        else:
            run.timings()
    return ms, events, accepted


off = make(False)
ms_off, _, _ = launches(off, False)
name_off = off.kernel_name()
off.close()
on = make(True)
ms_on, events, accepted = launches(on, True)
out = {"shape": f"sec11 k=2, {C} chains x {S} steps per launch, {IT} launches each",
       "kernel_off": name_off, "kernel_on": on.kernel_name(),
       "kernel_ms_off": {"median": float(np.median(ms_off)), "min": min(ms_off), "max": max(ms_off)},
       "kernel_ms_on": {"median": float(np.median(ms_on)), "min": min(ms_on), "max": max(ms_on)},
       "moved_per_accepted_step": events / max(accepted, 1), "moved_per_accepted_step_over_n": events / max(accepted, 1) / spec.n,
       "event_cap": S * spec.n, "max_events_per_chain_window": int(on.stats()["events"].max())}
# the five series calls over the last launch's window
rng = np.random.default_rng(1)
on.set_elections(rng.integers(0, 50, (spec.n, 2)), [(0, 1)])
area, edge_len, ext = G.unit_square_shapes(spec)
on.set_shapes(area, edge_len, ext)
on.set_localities(G.block_localities(spec, 8, 8))
calls = {"election_series": on.election_series, "shape_series": on.shape_series, "split_series": on.split_series,
         "sample_plans_every_5": lambda: on.sample_plans(every=5), "autocorr_4_lags": lambda: on.autocorr([1, 2, 5, S - 1])}
series = {}
for key, call in calls.items():
    call()  # the first call grows the run's buffers
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    series[key] = {"wall_ms_median": float(np.median(t))}
    if key.startswith("sample_plans"):
        k_ms, c_ms = on.sample_plans_ms()
        series[key].update(kernel_ms=k_ms, copy_ms=c_ms)
out["series_ms"] = series
on.close()
print(json.dumps(out), flush=True)
