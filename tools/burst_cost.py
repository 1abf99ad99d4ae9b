"""Cost of the short-bursts selection: python tools/burst_cost.py [chains] [bursts] [lengths]

sec11 40x40, k = 4 strips, the reference's tree_proposal parameters, population bound 0.1,
always_accept, 4096 ReCom chains with a move log; burst lengths 5, 20 and 100 (``lengths``: comma
separated).  Per length, after a warm-up burst, ``bursts`` bursts; each is timed as
  burst_ms          HIP-event time of the ReCom launch of the burst (fc_run_last_ms);
  election_wall_ms  host wall clock around fc_run_election_series on the burst's window, all chains:
                    the sibling that walks the same log with the same tallies;
  select_wall_ms    host wall clock around fc_run_burst_select (COUNT at 1/2, maximised) on the same
                    window without the rewind, and select_kernel_ms its kernel's HIP-event time;
  rewind_wall_ms /  the same for the call with FC_BURST_REWIND that ends the burst (it also rebuilds
  rewind_kernel_ms  the best plan and writes it into the run).
Each wall time ends in the call's own synchronise and includes its download of the chains' scalars
and the upload of the window (open_window).  Prints one JSON line and, with FC_BURST_COST_OUT set,
writes it there.  Measurements only: there is no pass / fail threshold."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import BurstMetric, FlipGraph, FlipRun, RunConfig

C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
IT = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LENGTHS = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [5, 20, 100]
K = 4
spec = G.sec11_graph()
init = spec.assignment_array(G.strip_plan(spec, K), list(range(K)))
_, (lo, hi) = G.population_bounds(spec.n, K, 0.1)
graph = FlipGraph(spec)
cols = np.random.default_rng(1).integers(0, 50, (spec.n, 2))
metric = BurstMetric("count", 0, 1, 1, 2, True)


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def stat(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def measure(b):
    cfg = RunConfig(k=K, labels=tuple(range(K)), proposal=_lib.FC_PROPOSE_RECOM, seed=0x5EED0011, pop_lo=lo, pop_hi=hi,
                    base=1.0, recom_pop_target=spec.n / K, recom_epsilon=0.05, recom_node_repeats=1,
                    diag_mask=_lib.FC_DIAG_SERIES, event_cap=b * spec.n + 64)
    run = FlipRun(graph, np.broadcast_to(init, (C, spec.n)), cfg)
    run.set_elections(cols, [(0, 1)])
    keys = ("burst_ms", "election_wall_ms", "select_wall_ms", "select_kernel_ms", "rewind_wall_ms", "rewind_kernel_ms")
    t = {key: [] for key in keys}
    events, best = 0, None
    for i in range(IT + 1):
        run.steps(b)
        run.sync()
        row = {"burst_ms": run.last_ms()}
        row["election_wall_ms"], _ = wall(run.election_series)
        row["select_wall_ms"], _ = wall(lambda: run.burst_select(metric))
        row["select_kernel_ms"] = run.burst_select_ms()
        ev = int(run.stats()["events"].sum())
        row["rewind_wall_ms"], sel = wall(lambda: run.burst_select(metric, rewind=True))
        row["rewind_kernel_ms"] = run.burst_select_ms()
        if i:  # the first burst grows the run's buffers and loads the code objects
            for key in keys:
                t[key].append(row[key])
            events += ev
            best = sel["best_score"]
    out = {key: stat(t[key]) for key in keys}
    out.update(burst_length=b, events_per_chain_burst=events / (IT * C), event_cap=b * spec.n + 64,
               kernel=run.kernel_name(), mean_best_score=float(best.mean()))
    run.close()
    return out


res = {"shape": f"sec11 k={K}, {C} ReCom chains, {IT} timed bursts per length after one warm-up burst",
       "metric": "COUNT 1/2 maximised over 2 random columns", "build_id": _lib.build_id(),
       "lengths": [measure(b) for b in LENGTHS]}
line = json.dumps(res)
print(line, flush=True)
if os.environ.get("FC_BURST_COST_OUT"):
    with open(os.environ["FC_BURST_COST_OUT"], "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
