#!/usr/bin/env python3
"""Time of the population tick against the forms the library offered before it.

In one process, hidden 256 x 2, demos on (each group's demo sets from the batched CEM, indexed),
P members of --envs-per-member envs:
  (pop)      one nav_act_tick_pop over P x envs_per_member envs, P actors, P rings;
  (separate) P nav_act_tick launches, one per member-sized VecEnv with its own actor and ring:
             the only form a sweep had before;
  (single)   one nav_act_tick over P x envs_per_member envs with one actor: what the population
             launch costs on top of is the member table's uniform loads.
HIP-event times after a warm-up of every form, the three forms interleaved, --repeats each; per
form the median, min and max. Every timed launch is a real training tick (the env state moves on).

python tools/population_tick_bench.py [--members 8] [--envs-per-member 8192] [--repeats 15]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))

import torch  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--envs-per-member", type=int, default=8192)
    ap.add_argument("--envs-per-group", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav.population import PopulationTrainer, sweep_grid
    from nav.trainer import VecTrainer
    P, epm = a.members, a.envs_per_member
    kw = dict(hidden=a.hidden, n_hidden=2, batch=epm, updates_per_step=0,
              envs_per_group=a.envs_per_group)
    members = sweep_grid(demo_factor=[10.0 + 10.0 * m for m in range(P)])
    pop = PopulationTrainer(members, envs_per_member=epm, **kw)
    seps = [VecTrainer(n_envs=epm, **kw) for _ in range(P)]
    single = VecTrainer(n_envs=P * epm, **kw)
    forms = {"pop": pop.collect, "single": single.collect,
             "separate": lambda: [t.collect() for t in seps]}
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, f in forms.items():
            ms[k].append(timed(f))
    res = {"members": P, "envs_per_member": epm, "hidden": a.hidden, "demos": True,
           **{k: summary(v) for k, v in ms.items()}}
    res["pop_over_separate"] = round(res["pop"]["median_ms"] / res["separate"]["median_ms"], 4)
    res["pop_over_single"] = round(res["pop"]["median_ms"] / res["single"]["median_ms"], 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
