"""Cost of the plan samples at the C2 shape:
    python tools/plans_cost.py [chains] [steps] [reps] [out.json]
sec11, 4096 chains (base bases[c % 10], alignment (c // 10) % 3), one window of 100,000 steps with
FC_DIAG_SERIES.  Reports, from one session: (a) the flip launch that fills the window (device ms);
(b) what a caller does without the device pass, reading every chain's log back with events();
(b') on 64 chains the numpy replay of that log at the same times, per chain; (c)
FlipRun.sample_plans(every=1000) of all chains (101 samples), in one call if the staged rows fit the
library's memory cap and in the fewest equal chain ranges otherwise; (c') the same call with plans
NULL (the walk, the scalars and the synchronisation); (c'') stride 100 on 512 chains.  (c), (c') and
(c'') are warmed up by two calls, then the median of `reps` calls with min and max, host clock
around the synchronising call; for (c) also the kernel's and the row copy's device time (HIP events,
medians over the same calls), the bytes the kernel stores and the rates they give.  Writes
profiles/plans_cost.json with the library's build id."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from flipcomplexityempirical_amd import _lib, graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig, sample_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
S = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 9
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "plans_cost.json")
HBM_PEAK = 8.0e12  # bytes / s, the roofline figure of DESIGN.md

spec = G.sec11_graph()
fg = FlipGraph(spec)
plans0 = [spec.assignment_array(G.sec11_plan(al, spec.nodes), [-1, 1]) for al in range(3)]
inits = np.stack([plans0[(c // 10) % 3] for c in range(C)])
bases = np.asarray([G.SEC11_BASES[c % 10] for c in range(C)])
_, (lo, hi) = G.population_bounds(spec.n, 2, 0.1)
cfg = RunConfig(seed=0x5EED0002, pop_lo=lo, pop_hi=hi, diag_mask=_lib.FC_DIAG_WAIT | _lib.FC_DIAG_SERIES,
                event_cap=S + 1)
run = FlipRun(fg, inits, cfg, bases=bases)

t = time.perf_counter()
run.steps(S)
run.sync()
flip_host_s = time.perf_counter() - t
flip_ms = run.last_ms()
st = run.stats()
events = int(st["events"].sum())
npad = (spec.n + 15) // 16 * 16


def stat(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x)), "reps": len(x)}


def timed(read):
    """Two warm-up calls, then REPS timed ones: the last result, the host seconds, and the device ms
    of the kernel and the row copy of every timed call."""
    for _ in range(2):
        out = read()
    host, kern, copy = [], [], []
    for _ in range(REPS):
        t = time.perf_counter()
        out = read()
        host.append(time.perf_counter() - t)
        k_ms, c_ms = run.sample_plans_ms()
        kern.append(k_ms)
        copy.append(c_ms)
    return out, stat(host), kern, copy


# (c): every chain, stride 1000, in the fewest equal chain ranges the memory cap admits
times = sample_times(0, S, 1000)
ranges = 1
while True:
    per = -(-C // ranges)
    try:
        run.sample_plans(times, c0=0, nc=per)
        break
    except ValueError as err:
        if "split the call" not in str(err) or per == 1:
            raise
        ranges *= 2
bounds = [(c0, min(per, C - c0)) for c0 in range(0, C, per)]


def sample_all():
    parts = [run.sample_plans(times, c0=c0, nc=nc) for c0, nc in bounds]
    return parts[0] if len(parts) == 1 else {key: (parts[0][key] if key == "times" else np.concatenate(
        [p[key] for p in parts])) for key in parts[0]}


out, plans_s, kern_ms, copy_ms = timed(sample_all)
assert np.array_equal(out["plans"][:, -1], run.state()) and np.array_equal(out["pops"][:, -1], run.pops())
assert np.array_equal(out["plans"][:, 0], inits) and (out["dist0"][:, 0] == 0).all()
assert (out["pops"].sum(axis=2) == spec.n).all()
_, noplans_s, kern_np_ms, _ = timed(lambda: run.sample_plans(times, plans=False))
dense_times = sample_times(0, S, 100)
C2 = min(512, C)
dense, dense_s, kern_d_ms, copy_d_ms = timed(lambda: run.sample_plans(dense_times, c0=0, nc=C2))

# (b): the log of every chain read back; (b'): replayed in numpy at the same times, 64 chains
t = time.perf_counter()
log_bytes = 0
logs = []
for c in range(C):
    ev = run.events(c)
    log_bytes += ev.nbytes
    if c < 64:
        logs.append(ev)
readback_s = time.perf_counter() - t
t = time.perf_counter()
for c, ev in enumerate(logs):
    a = inits[c].copy()
    rows = np.zeros((times.size, spec.n), dtype=np.int8)
    lo_i = 0
    for j, hi_i in enumerate(np.searchsorted(ev["t"], times, side="right")):
        a[ev["v"][lo_i:hi_i]] = ev["target"][lo_i:hi_i]
        lo_i = hi_i
        rows[j] = a
    assert np.array_equal(rows, out["plans"][c])
replay_s = (time.perf_counter() - t) / max(len(logs), 1)

row_bytes = C * times.size * npad  # what the kernel stores for (c): the staged rows
scalar_bytes = C * times.size * 8 * (3 + cfg.k)
kern_s = float(np.median(kern_ms)) / 1e3
copy_s = float(np.median(copy_ms)) / 1e3
res = {"build_id": _lib.build_id(),
       "workload": f"sec11 C2 shape: {C} chains x {S} steps, one window; samples every 1000 yields ({times.size})",
       "chains": C, "steps": S, "events": events, "log_bytes": log_bytes, "samples": int(times.size),
       "flip_launch_ms": flip_ms, "flip_launch_host_s": flip_host_s,
       "events_readback_s": readback_s,
       "numpy_replay_s_per_chain": replay_s, "numpy_replay_chains": len(logs),
       "sample_plans_s": plans_s, "sample_plans_calls": len(bounds),
       "sample_plans_kernel_ms": stat(kern_ms), "sample_plans_copy_ms": stat(copy_ms),
       "plans_bytes_host": int(out["plans"].nbytes), "kernel_store_bytes": int(row_bytes + scalar_bytes),
       "kernel_store_bytes_per_s": (row_bytes + scalar_bytes) / kern_s if kern_s else None,
       "kernel_store_over_hbm_peak": (row_bytes + scalar_bytes) / kern_s / HBM_PEAK if kern_s else None,
       "copy_bytes_per_s": out["plans"].nbytes / copy_s if copy_s else None,
       "sample_plans_no_plans_s": noplans_s, "sample_plans_no_plans_kernel_ms": stat(kern_np_ms),
       "sample_plans_stride100_512_s": dense_s, "sample_plans_stride100_512_kernel_ms": stat(kern_d_ms),
       "sample_plans_stride100_512_copy_ms": stat(copy_d_ms), "stride100_chains": C2,
       "stride100_samples": int(dense_times.size), "stride100_plans_bytes": int(dense["plans"].nbytes),
       "sample_over_readback": plans_s["median"] / readback_s,
       "mean_dist0_last": float(out["dist0"][:, -1].mean())}
print(json.dumps(res))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
