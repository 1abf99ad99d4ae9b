"""Cost of the seed plans: python tools/seed_plans_cost.py [out.json] [calls]

4096 plans on sec11 (the 40 x 40 lattice, n = 1596) at k = 2, 4 and 8 with bounds within 1 % and within 5 % of
ideal, and 1024 plans on the 100 x 80 grid (n = 8000, the LDS limit) at k = 2 within 1 %; parameters
at their defaults (node_repeats 1, max_attempts 256, max_restarts 16).  Per shape, over `calls`
(10) calls after one warm-up call, each call over its own range of plan ids:
  kernel_ms                 HIP-event time of the kernel (fc_graph_seed_plans kernel_ms): median, min, max;
  wall_ms                   host wall clock around the call (table upload, launch, copy back): median;
  trees / attempts / restarts per plan: mean and max;  plans_restarted: plans with restarts > 0,
                            i.e. plans in which some level used up max_attempts;
  failed                    plans with ok = 0;   distinct: distinct rows among the ok plans;
  kernel_ms_per_tree        kernel_ms (median) over the mean number of trees a wave drew in a call.
Beside them the yardstick: a plain ReCom run (sec11 k = 2, the reference's tree_proposal parameters,
4096 chains x 20 steps per launch), launched alternately with the sec11 k = 2 within-1 % seed calls
in the same process: its kernel ms per launch over the mean growth of a chain's spanning-tree
counter (bfs_levels) in that launch.  A level-0 seed tree spans the whole graph, as a k = 2 ReCom
tree does.  Measurements only: there is no pass / fail threshold."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig

OUT = sys.argv[1] if len(sys.argv) > 1 else None
IT = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SEED = 0x5EED0011
RECOM_CHAINS, RECOM_STEPS = 4096, 20


def spread(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


class Shape:
    def __init__(self, name, graph, spec, k, pct, n_plans):
        self.name, self.graph, self.spec, self.k, self.pct, self.n_plans = name, graph, spec, k, pct, n_plans
        self.bounds = G.population_bounds(int(spec.pop.astype(np.int64).sum()), k, pct)[1]
        self.ms, self.wall, self.stats, self.rows = [], [], [], set()
        self.calls = 0

    def call(self):
        """One call over the next range of plan ids; the first is the warm-up and is not kept."""
        t0 = time.perf_counter()
        plans, st = self.graph.seed_plans(self.k, self.n_plans, pop_bounds=self.bounds, seed=SEED,
                                          plan_id_offset=self.calls * self.n_plans, strict=False, timing=True)
        wall = (time.perf_counter() - t0) * 1e3
        self.calls += 1
        if self.calls == 1:
            return
        self.ms.append(st["kernel_ms"])
        self.wall.append(wall)
        self.stats.append(st)
        self.rows.update(hash(p.tobytes()) for p, ok in zip(plans, st["ok"]) if ok)

    def report(self):
        cat = {f: np.concatenate([s[f] for s in self.stats]) for f in ("attempts", "trees", "restarts", "ok")}
        trees_per_call = float(np.mean([s["trees"].mean() for s in self.stats]))
        out = {"shape": self.name, "k": self.k, "within": self.pct, "bounds": list(self.bounds), "plans_per_call": self.n_plans,
               "calls": len(self.ms), "kernel": self.stats[0]["kernel"], "kernel_ms": spread(self.ms),
               "wall_ms": spread(self.wall)}
        for f in ("trees", "attempts", "restarts"):
            out[f + "_per_plan"] = {"mean": float(cat[f].mean()), "max": int(cat[f].max())}
        out["plans_restarted"] = int((cat["restarts"] > 0).sum())
        out["failed"] = int((cat["ok"] == 0).sum())
        out["plans"] = int(len(cat["ok"]))
        out["distinct"] = len(self.rows)
        out["kernel_ms_per_tree"] = float(np.median(self.ms)) / trees_per_call
        return out


sec11 = G.sec11_graph()
g_sec11 = FlipGraph(sec11)
big = G.grid_graph(100, 80)
shapes = [Shape("sec11 40x40", g_sec11, sec11, k, pct, 4096) for k in (2, 4, 8) for pct in (0.01, 0.05)]
shapes.append(Shape("grid 100x80", FlipGraph(big), big, 2, 0.01, 1024))

# the yardstick, alternating with the first shape (sec11 k = 2 within 1 %)
plans3 = [sec11.assignment_array(G.sec11_plan(al, sec11.nodes), [-1, 1]) for al in range(3)]
_, (lo, hi) = G.population_bounds(sec11.n, 2, 0.1)
cfg = RunConfig(proposal=_lib.FC_PROPOSE_RECOM, seed=0x5EED0010, pop_lo=lo, pop_hi=hi, base=1.0,
                recom_pop_target=sec11.n / 2, recom_epsilon=0.05, recom_node_repeats=1, diag_mask=0)
recom = FlipRun(g_sec11, np.stack([plans3[c % 3] for c in range(RECOM_CHAINS)]), cfg)
r_ms, r_trees = [], []
for i in range(IT + 1):
    shapes[0].call()
    t0 = recom.stats()["bfs_levels"].astype(np.int64)
    recom.steps(RECOM_STEPS)
    recom.sync()
    ms = float(recom.timings()[-1])
    if i:
        r_ms.append(ms)
        r_trees.append(float((recom.stats()["bfs_levels"].astype(np.int64) - t0).mean()))
yard = {"shape": f"sec11 k=2 ReCom run, {RECOM_CHAINS} chains x {RECOM_STEPS} steps per launch, {IT} launches",
        "kernel": recom.kernel_name(), "kernel_ms": spread(r_ms), "trees_per_chain_per_launch": float(np.mean(r_trees)),
        "kernel_ms_per_tree": float(np.median(r_ms)) / float(np.mean(r_trees))}
recom.close()
for s in shapes[1:]:
    for _ in range(IT + 1):
        s.call()
out = {"defaults": {"node_repeats": 1, "max_attempts": 256, "max_restarts": 16}, "seed": SEED,
       "shapes": [s.report() for s in shapes], "recom_yardstick": yard}
text = json.dumps(out, indent=1)
if OUT:
    with open(OUT, "w") as f:
        f.write(text + "\n")
print(json.dumps(out), flush=True)
