"""Cost of the locality-splits series at the C2 shape:
    python tools/split_cost.py [chains] [steps] [reps] [out.json]
sec11, 4096 chains (base bases[c % 10], alignment (c // 10) % 3), one window of 100,000 steps with
FC_DIAG_SERIES, localities = 4 x 4 blocks (100).  Reports, from one session: (a) the flip launch
that fills the window (device ms), (b) reading every chain's log back with events() -- the only way
to these statistics without the device pass --, (c) the device pass, FlipRun.split_series of all
chains, and (d) FlipRun.election_series with one election on the same run: (c) and (d) warmed up by
two calls, then the median of `reps` calls with min and max, host clock around the synchronising
call; (c) also as the raw call with every output pointer NULL (no copy of the results).  Writes
profiles/split_cost.json with the library's build id."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from flipcomplexityempirical_amd import _lib, graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
S = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 9
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "split_cost.json")

spec = G.sec11_graph()
fg = FlipGraph(spec)
plans = [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]
inits = np.stack([plans[(c // 10) % 3] for c in range(C)])
bases = np.asarray([G.SEC11_BASES[c % 10] for c in range(C)])
_, (lo, hi) = G.population_bounds(spec.n, 2, 0.1)
cfg = RunConfig(seed=0x5EED0002, pop_lo=lo, pop_hi=hi, diag_mask=_lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES,
                event_cap=S + 1)
run = FlipRun(fg, inits, cfg, bases=bases)
node_loc = G.block_localities(spec, 4, 4)
n_loc = int(node_loc.max()) + 1
run.set_localities(node_loc)
cols = np.random.default_rng(1).integers(0, 100, (spec.n, 2))
total = int(cols.sum())
run.set_elections(cols, [(0, 1)], np.linspace(-total // 4, total // 4, 16).astype(np.int64))

t = time.perf_counter()
run.steps(S)
run.sync()
flip_host_s = time.perf_counter() - t
flip_ms = run.last_ms()
st = run.stats()
events = int(st["events"].sum())


def timed(read):
    for _ in range(2):
        out = read()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        out = read()
        times.append(time.perf_counter() - t)
    return out, {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times)), "reps": REPS}


out, split_s = timed(run.split_series)
assert (out["splits_hist"].sum(axis=-1) == S + 1).all() and (out["excess_hist"].sum(axis=-1) == S + 1).all()
assert np.array_equal(out["cells_now"].sum(axis=1), run.pops())
assert (out["parts_sum"].sum(axis=1) == out["dlocs_sum"].sum(axis=1)).all()
assert (out["split_sum"].sum(axis=1) == (out["splits_hist"] * np.arange(n_loc + 1)).sum(axis=1)).all()
# the same call with every output pointer NULL: the window, the kernel and the synchronisation,
# without the copy of the results (cells_now is most of it) to the host
null_call = lambda: _lib.check(_lib.load().fc_run_split_series(run.handle, 0, C, *([None] * 7)), "fc_run_split_series")
_, split_null_s = timed(null_call)
el, election_s = timed(run.election_series)
assert (el["seats_hist"].sum(axis=-1) == S + 1).all()

t = time.perf_counter()
log_bytes = 0
for c in range(C):
    log_bytes += run.events(c).nbytes
readback_s = time.perf_counter() - t

res = {"build_id": _lib.build_id(), "workload": f"sec11 C2 shape: {C} chains x {S} steps, one window, 4 x 4 blocks "
                                                f"({n_loc} localities); 2 columns, 1 election, 16 gap edges",
       "chains": C, "steps": S, "events": events, "log_bytes": log_bytes, "n_loc": n_loc, "x_max": out["x_max"],
       "flip_launch_ms": flip_ms, "flip_launch_host_s": flip_host_s,
       "events_readback_s": readback_s,
       "split_series_s": split_s,
       "split_series_no_outputs_s": split_null_s,
       "election_series_s": election_s,
       "split_series_events_per_s": events / split_s["median"],
       "split_over_election": split_s["median"] / election_s["median"],
       "mean_splits_now": float(out["splits_now"].mean()),
       "outputs_bytes_per_chain": int(sum(v[0].nbytes for k_, v in out.items()
                                          if isinstance(v, np.ndarray) and k_ != "yields"))}
print(json.dumps(res))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
