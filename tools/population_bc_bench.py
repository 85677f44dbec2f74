#!/usr/bin/env python3
"""Time of the population learner with demonstrations against the members' own updates.

In one process, P members at batch B, hidden 256 x 2, rings filled with random rows and a tail of
random demonstration rows behind each; every member has demo_fraction and bc_weight on. One timed
unit is one policy epoch (mix, critic phase, BC actor phase, soft updates) plus one critic-only
epoch (mix, critic phase):
  (batched_bc)  PopulationLearner.update: one launch per kernel for all members, one
                nav_td3_mix_idx_pop per epoch and nav_td3_actor_rows_bc_pop on policy epochs;
  (members_bc)  every member's td3_update (TD3._update) in turn on one stream: what
                learner="members" does;
  (batched)     the batched learner of members without the keys on the same rings: the plain
                epochs, for the ratio.
HIP-event times after 3 warm-up rounds of every form, the forms interleaved, --repeats each; per
form the median, min and max, and the host's wall time to issue one unit (no synchronisation
inside). The gate: the batched BC median is below the members' BC median of the same run.

python tools/population_bc_bench.py [--members 8] [--batch 4096] [--repeats 15]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))

import torch  # noqa: E402


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--tail", type=int, default=2388, help="demonstration rows behind each ring")
    ap.add_argument("--demo-fraction", type=float, default=0.25)
    ap.add_argument("--bc-weight", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav import config as K
    from nav.population import PopulationLearner
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    P, B, dev = a.members, a.batch, "cuda"

    def ring(seed):
        r = ReplayRing(a.capacity, dev, tail=a.tail)
        g = torch.Generator().manual_seed(seed)
        rows = torch.randn(a.capacity + a.tail, 8, generator=g)
        rows[:, 7] = (torch.rand(a.capacity + a.tail, generator=g) < 0.05).float()
        r.storage.copy_(rows.to(dev))
        r.advance(a.capacity)
        return r

    def learner(m, bc, splits=None):
        kw = dict(demo_fraction=a.demo_fraction, bc_weight=a.bc_weight) if bc else {}
        cfg = K.TD3Config(batch_size=B, num_epochs=2, policy_update_delay=2,
                          critic_lr=1e-3 / (m + 1),
                          net=K.NetConfig(hidden=a.hidden, n_hidden=a.n_hidden), **kw)
        return TD3(cfg, device=dev, seed=100 + m, wgrad_splits=splits)

    rings = [ring(m) for m in range(P)]
    batched_bc = PopulationLearner([learner(m, True) for m in range(P)], rings)
    batched = PopulationLearner([learner(m, False) for m in range(P)], rings)
    members = [learner(m, True) for m in range(P)]
    for t in members:
        t._workspace(B)
    assert batched_bc.bc_table is not None and batched.bc_table is None

    def members_bc():
        for t, r in zip(members, rings):
            t.td3_update(r, 2)

    # epochs 0 (policy) and 1 (critic only) of an update of 2: the timed unit
    forms = {"batched_bc": lambda: batched_bc.update(2), "members_bc": members_bc,
             "batched": lambda: batched.update(2)}
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    ms, issue = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, f in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            t0 = time.perf_counter()
            f()
            issue[k].append((time.perf_counter() - t0) * 1e3)
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    res = {"members": P, "batch": B, "hidden": a.hidden, "n_hidden": a.n_hidden,
           "demo_fraction": a.demo_fraction, "bc_weight": a.bc_weight, "tail": a.tail,
           "b_demo": members[0].b_demo(),
           "batched_wgrad_splits": list(batched_bc.wgrad_splits),
           "members_wgrad_splits": [members[0].splits_c, members[0].splits_a],
           "mix_launches": {"batched_bc": batched_bc.mix_launches, "batched": batched.mix_launches,
                            "members_bc_each": members[0].mix_launches},
           **{k: summary(v) for k, v in ms.items()},
           "host_issue_ms": {k: round(statistics.median(v), 4) for k, v in issue.items()}}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res["batched_bc_over_members_bc"] = round(med("batched_bc") / med("members_bc"), 4)
    res["batched_bc_over_batched"] = round(med("batched_bc") / med("batched"), 4)
    res["gate"] = bool(med("batched_bc") < med("members_bc"))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["gate"] else 1


if __name__ == "__main__":
    sys.exit(main())
