#!/usr/bin/env python3
"""Time of the population learner against the forms the library offered before it.

In one process, P members at batch B, hidden 256 x 2, rings filled with random rows; one timed
unit is one critic-only epoch plus one policy epoch (critic phase, actor phase, soft updates):
  (batched)   PopulationLearner.update: one launch per kernel for all members;
  (members1)  every member's td3_update in turn on one stream: the form a sweep had before;
  (members4)  the same, the members round-robin over 4 side streams (PopulationTrainer.learn);
  (single)    one lone TD3 at batch P x B: context only, the same rows as one learner's.
HIP-event times after 3 warm-up rounds of every form, the forms interleaved, --repeats each; per
form the median, min and max, and the host's wall time to issue one unit (no synchronisation
inside). `members*` run with their own split counts (nav_mlp_wgrad_splits), as a sweep did.

python tools/population_learner_bench.py [--members 8] [--batch 4096] [--repeats 15]
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
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav import config as K
    from nav.population import PopulationLearner
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    P, B, dev = a.members, a.batch, "cuda"

    def ring(seed):
        r = ReplayRing(a.capacity, dev)
        g = torch.Generator().manual_seed(seed)
        rows = torch.randn(a.capacity, 8, generator=g)
        rows[:, 7] = (torch.rand(a.capacity, generator=g) < 0.05).float()
        r.rows.copy_(rows.to(dev))
        r.advance(a.capacity)
        return r

    def learner(m, batch):
        cfg = K.TD3Config(batch_size=batch, num_epochs=2, policy_update_delay=2,
                          critic_lr=1e-3 / (m + 1),
                          net=K.NetConfig(hidden=a.hidden, n_hidden=a.n_hidden))
        return TD3(cfg, device=dev, seed=100 + m)

    rings = [ring(m) for m in range(P)]
    batched = PopulationLearner([learner(m, B) for m in range(P)], rings)
    members = [learner(m, B) for m in range(P)]
    for t in members:
        t._workspace(B)
    single = learner(0, P * B)
    side = [torch.cuda.Stream() for _ in range(4)]
    main_s = torch.cuda.current_stream()
    ticked, done = torch.cuda.Event(), [torch.cuda.Event() for _ in side]

    def members1():
        for t, r in zip(members, rings):
            t.td3_update(r, 2)

    def members4():
        ticked.record(main_s)
        for s in side:
            s.wait_event(ticked)
        for m, (t, r) in enumerate(zip(members, rings)):
            t.td3_update(r, 2, stream=side[m % 4])
        for s, e in zip(side, done):
            e.record(s)
            main_s.wait_event(e)

    # epochs 0 (policy) and 1 (critic only) of td3_update(.., 2): the timed unit
    forms = {"batched": lambda: batched.update(2), "members1": members1, "members4": members4,
             "single": lambda: single.td3_update(rings[0], 2)}
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
           "batched_wgrad_splits": list(batched.wgrad_splits),
           "members_wgrad_splits": [members[0].splits_c, members[0].splits_a],
           "batched_split_twins": int(P * B <= 2048), "members_split_twins": int(B <= 2048),
           **{k: summary(v) for k, v in ms.items()},
           "host_issue_ms": {k: round(statistics.median(v), 4) for k, v in issue.items()}}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res["batched_over_members1"] = round(med("batched") / med("members1"), 4)
    res["batched_over_members4"] = round(med("batched") / med("members4"), 4)
    res["batched_over_single"] = round(med("batched") / med("single"), 4)
    res["gate"] = bool(med("batched") <= med("members1") and med("batched") <= med("members4"))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["gate"] else 1


if __name__ == "__main__":
    sys.exit(main())
