#!/usr/bin/env python3
"""Cost of resets to demonstration states: the trainer's step at demo_reset_prob 0 (off: the
parent's launches, nothing of the feature) and 0.25 (one nav_demo_reset launch after every tick),
and the entry point alone.

In one process, BASELINE configuration 3: 65 536 envs, hidden 256 x 2, batch 32 768, two updates
per step. One timed unit is --unit consecutive VecTrainer.step() calls (HIP events around the
unit, divided by --unit: one step is too short for an event pair), the two trainers interleaved,
--repeats units each after 3 warm-up units of both; per form the median, min and max per step and
the host's wall time to issue one step. Then nav_demo_reset alone on the 0.25 trainer's env, the
same way (an event pair around one call: launch overhead included; the kernel's own time comes
from a kernel trace, e.g. rocprofv3 --kernel-trace --stats -- python tools/demo_reset_bench.py
--repeats 3): on the flags the last tick left, and with every env flagged at probability 1 (the
worst case: every lane draws, loads and stores). There is no gate: the figures go to
profiles/demo_resets.txt. Starts no other process; run it under a time limit, e.g.

timeout -k 10 400 python tools/demo_reset_bench.py [--n-envs 65536] [--batch 32768] [--prob 0.25]
    [--unit 20] [--repeats 15] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))

import torch  # noqa: E402

from per_bench import summary, timed  # noqa: E402  (the same event-pair timing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--prob", type=float, default=0.25)
    ap.add_argument("--unit", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav.trainer import VecTrainer
    kw = dict(n_envs=a.n_envs, hidden=a.hidden, n_hidden=a.n_hidden, batch=a.batch,
              updates_per_step=2, envs_per_group=min(1024, a.n_envs))
    off = VecTrainer(**kw, demo_reset_prob=0.0)
    on = VecTrainer(**kw, demo_reset_prob=a.prob)

    def unit(tr):
        def run():
            for _ in range(a.unit):
                tr.step()
        return run

    forms = {"p0": unit(off), f"p{a.prob:g}": unit(on)}
    ms, issue = timed(forms, a.repeats)
    per_step = {k: [x / a.unit for x in v] for k, v in ms.items()}
    steps = a.unit * (3 + a.repeats)
    assert off.env.demo_reset_launches == 0 and off.env.demo_resets is None
    assert on.env.demo_reset_launches == steps == on.steps
    ended = on.env.flags.bitwise_and(8).ne(0).float().mean().item()

    # the entry point alone, on the env of the trainer that has the set
    env = on.env
    keep = {k: getattr(env, k).clone() for k in ("state", "flags", "demo_resets")}
    d = dict(env._dreset)
    full = dict(d, prob=1.0)

    def all_flagged():
        env._dreset = full
        env._demo_reset()
        env._dreset = d

    kms, _ = timed({"nav_demo_reset_last_tick": env._demo_reset}, a.repeats)
    env.flags.fill_(8)
    kms2, _ = timed({"nav_demo_reset_all_p1": all_flagged}, a.repeats)
    kms.update(kms2)
    for k, v in keep.items():
        getattr(env, k).copy_(v)
    torch.cuda.synchronize()

    res = {"n_envs": a.n_envs, "hidden": a.hidden, "n_hidden": a.n_hidden, "batch": a.batch,
           "prob": a.prob, "unit_steps": a.unit, "steps_per_trainer": steps,
           "demo_reset_share": round(on.env.demo_reset_share(), 6),
           "taken": int(keep["demo_resets"].sum().item()),
           "episodes_started": int(on.env.episodes.sum().item()) - 5 * a.n_envs,
           "ended_fraction_last_tick": round(ended, 5),
           "ms_per_step": {k: summary(v) for k, v in per_step.items()},
           "host_issue_ms_per_step": {k: round(statistics.median(v) / a.unit, 4)
                                      for k, v in issue.items()},
           "kernels": {k: summary(v) for k, v in kms.items()}}
    p0, p1 = (res["ms_per_step"][k]["median_ms"] for k in forms)
    res["added_ms_per_step"] = round(p1 - p0, 4)
    res["on_over_off"] = round(p1 / p0, 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"Resets to demonstration states: VecTrainer.step(), {a.n_envs} envs, "
                    f"{a.hidden} x {a.n_hidden}, batch {a.batch}, 2 updates per step, one MI355X; "
                    f"medians of {a.repeats} units of {a.unit} steps, per step, the two trainers "
                    "interleaved in one process (tools/demo_reset_bench.py).\n\n")
            for k in forms:
                v = res["ms_per_step"][k]
                f.write(f"  {k:<6} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f}); host issue "
                        f"{res['host_issue_ms_per_step'][k]:.4f} ms\n")
            f.write(f"  on / off {res['on_over_off']:.4f}, added {res['added_ms_per_step']:.4f} ms "
                    f"per step\n  after {steps} steps: {res['taken']} of "
                    f"{res['episodes_started']} started episodes on a demonstration state, "
                    f"demo_reset_share {res['demo_reset_share']}; the last tick ended "
                    f"{100 * ended:.2f} % of the envs\n\n"
                    "The entry point alone (event time around one call, launch overhead "
                    "included):\n")
            for k, v in res["kernels"].items():
                f.write(f"  {k:<26} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f})\n")
            f.write("\n" + json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
