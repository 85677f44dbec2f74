#!/usr/bin/env python3
"""Cost of multi-step returns: the learner's epochs at n_step 1 (off), 3, 8 and 3 with
prioritised replay, and the feature's own launches.

In one process, hidden 256 x 2 at batch 32 768 on a full ring of 262 144 random rows written by
65 536 envs (stride 65 536: four ticks deep), one row in ten cut (half of those done). One timed
unit is one policy epoch (critic phase, actor phase, soft updates) plus one critic-only epoch:
  (n1)      TD3.td3_update with n_step = 1: the plain launches, nothing of the feature;
  (n3, n8)  per epoch one nav_nstep_rows, then the unchanged critic launch on the staged rows;
  (n3_per)  n_step = 3 with per_alpha on: nav_per_sums, nav_per_sample, nav_nstep_rows on the
            sampled indices, nav_td3_critic_rows_w on the staged rows, nav_per_update.
HIP-event times after 3 warm-up rounds of all forms, the forms interleaved, --repeats each; per
form the median, min and max and the host's wall time to issue one unit. Then nav_nstep_rows at
several n_step and nav_nstep_stamp alone, the same way (an event pair around one call: launch
overhead included; the kernels' own times come from a kernel trace). There is no gate: the figures
go to profiles/nstep_returns.txt. Starts no other process; run it under a time limit, e.g.

timeout -k 10 300 python tools/nstep_bench.py [--batch 32768] [--capacity 262144]
    [--stride 65536] [--repeats 15] [--out FILE]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=262144)
    ap.add_argument("--stride", type=int, default=65536)
    ap.add_argument("--per-alpha", type=float, default=0.6)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav import config as K
    from nav._lib import lib, ptr, stream_handle
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    B, dev, cap = a.batch, "cuda", a.capacity
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(cap, 8, generator=g)
    u = torch.rand(cap, generator=g)
    rows[:, 7] = (u < 0.05).float()
    cut = (u < 0.10).to(torch.uint8)

    def ring(n_step, priorities=False):
        r = ReplayRing(cap, dev, priorities=priorities, cuts=n_step > 1)
        r.stride = a.stride
        r.rows.copy_(rows.to(dev))
        base = r.advance(cap)
        r.stamp(base, cap)
        if r.cut is not None:
            r.cut.copy_(cut.to(dev))
        return r

    def learner(n_step, alpha=0.0):
        cfg = K.TD3Config(batch_size=B, num_epochs=2, policy_update_delay=2, per_alpha=alpha,
                          n_step=n_step, net=K.NetConfig(hidden=a.hidden, n_hidden=a.n_hidden))
        return TD3(cfg, device=dev, seed=100)

    sets = {"n1": (1, 0.0), "n3": (3, 0.0), "n8": (8, 0.0), "n3_per": (3, a.per_alpha)}
    rings = {k: ring(n, alpha != 0) for k, (n, alpha) in sets.items()}
    learners = {k: learner(n, alpha) for k, (n, alpha) in sets.items()}
    # epochs 0 (policy) and 1 (critic only) of an update of 2: the timed unit
    forms = {k: (lambda k=k: learners[k].td3_update(rings[k], 2)) for k in sets}
    ms, issue = timed(forms, a.repeats)
    assert learners["n1"].nstep_launches == 0 and rings["n1"].cut is None
    assert learners["n3"].nstep_launches == 2 * (3 + a.repeats)
    # the feature's own launches
    L, s = lib(), stream_handle()
    t3, r3 = learners["n3"], rings["n3"]
    d3, seed = r3.desc(), (100, 0)
    rd = C.byref(d3)
    flags = torch.full((min(65536, cap),), 8, dtype=torch.uint8, device=dev)
    kernels = {f"nav_nstep_rows_n{n}": (lambda n=n: L.nav_nstep_rows(
        rd, ptr(r3.cut), cap, 0, a.stride, n, 0.99, B, None, *seed, 7, ptr(t3.staged),
        ptr(t3.steps), s)) for n in (1, 2, 3, 8, K.NSTEP_MAX)}
    kernels["nav_nstep_rows_n3_idx"] = lambda: L.nav_nstep_rows(
        rd, ptr(r3.cut), cap, 0, a.stride, 3, 0.99, B, ptr(learners["n3_per"].idx_c), *seed, 7,
        ptr(t3.staged), ptr(t3.steps), s)
    kernels[f"nav_nstep_stamp_{flags.shape[0]}"] = lambda: L.nav_nstep_stamp(
        ptr(r3.cut), cap, 0, flags.shape[0], ptr(flags), s)
    kernels["nav_replay_sample"] = lambda: L.nav_replay_sample(
        rd, cap, B, None, *seed, 14, ptr(t3.staged), s)  # the one-row gather, for scale
    keep = r3.cut.clone()  # (the stamp form writes the marks: put them back after)
    kms, _ = timed(kernels, a.repeats)
    r3.cut.copy_(keep)
    steps = {k: torch.bincount(learners[k].steps, minlength=sets[k][0] + 1).tolist()[1:]
             for k in sets if sets[k][0] > 1}
    res = {"batch": B, "hidden": a.hidden, "n_hidden": a.n_hidden, "capacity": cap,
           "stride": a.stride, "cut_fraction": round(float(cut.float().mean()), 4),
           "horizons_last_epoch": steps,
           **{k: summary(v) for k, v in ms.items()},
           "host_issue_ms": {k: round(statistics.median(v), 4) for k, v in issue.items()},
           "kernels": {k: summary(v) for k, v in kms.items()}}
    base = res["n1"]["median_ms"]
    res["added_ms"] = {k: round(res[k]["median_ms"] - base, 4) for k in sets if k != "n1"}
    res["over_n1"] = {k: round(res[k]["median_ms"] / base, 4) for k in sets if k != "n1"}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"Multi-step returns: one policy epoch + one critic-only epoch, {a.hidden} x "
                    f"{a.n_hidden}, batch {B}, ring {cap} rows full, stride {a.stride}, one "
                    f"MI355X; medians of {a.repeats}, the forms interleaved in one process "
                    "(tools/nstep_bench.py).\n\n")
            for k in sets:
                v = res[k]
                f.write(f"  {k:<7} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f}); host issue {res['host_issue_ms'][k]:.4f} ms\n")
            for k in res["added_ms"]:
                f.write(f"  {k} / n1 {res['over_n1'][k]:.4f}, added {res['added_ms'][k]:.4f} ms "
                        "per unit\n")
            f.write(f"  horizons 1 .. n_step of the last epoch's batch: {steps}\n\n"
                    "Each entry point alone (event time around one call, launch overhead "
                    "included):\n")
            for k, v in res["kernels"].items():
                f.write(f"  {k:<24} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f})\n")
            f.write("\n" + json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
