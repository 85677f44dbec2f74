#!/usr/bin/env python3
"""Cost of prioritised replay: the learner's epochs with it on and off, and its own launches.

In one process, hidden 256 x 2 at batch 32 768 on a full ring of 262 144 random rows. One timed
unit is one policy epoch (critic phase, actor phase, soft updates) plus one critic-only epoch:
  (per)    TD3.td3_update with per_alpha on: per epoch nav_per_sums, nav_per_sample,
           nav_td3_critic_rows_w, the weight gradients, reduce + Adam, nav_per_update, and the
           plain actor launch on the policy epoch;
  (plain)  the same update with per_alpha = 0 on a ring of the same rows.
The priorities start at the stamp and are whatever the timed epochs themselves leave. HIP-event
times after 3 warm-up rounds of both forms, the forms interleaved, --repeats each; per form the
median, min and max and the host's wall time to issue one unit. Then each nav_per_* entry point
alone, the same way. There is no gate: the figures go to profiles/per_replay.txt.

python tools/per_bench.py [--batch 32768] [--capacity 262144] [--repeats 15] [--out FILE]
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


def timed(forms, repeats, warm=3):
    """{name: (event ms, host issue ms)} of the callables, interleaved."""
    for _ in range(warm):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    ms, issue = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(repeats):
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
    return ms, issue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=262144)
    ap.add_argument("--per-alpha", type=float, default=0.6)
    ap.add_argument("--per-beta", type=float, default=0.4)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nav import config as K
    from nav._lib import lib, ptr, stream_handle
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    B, dev = a.batch, "cuda"
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(a.capacity, 8, generator=g)
    rows[:, 7] = (torch.rand(a.capacity, generator=g) < 0.05).float()

    def ring(priorities):
        r = ReplayRing(a.capacity, dev, priorities=priorities)
        r.rows.copy_(rows.to(dev))
        base = r.advance(a.capacity)
        r.stamp(base, a.capacity)
        return r

    def learner(alpha):
        cfg = K.TD3Config(batch_size=B, num_epochs=2, policy_update_delay=2, per_alpha=alpha,
                          per_beta=a.per_beta,
                          net=K.NetConfig(hidden=a.hidden, n_hidden=a.n_hidden))
        return TD3(cfg, device=dev, seed=100)

    r_per, r_plain = ring(True), ring(False)
    t_per, t_plain = learner(a.per_alpha), learner(0.0)
    # epochs 0 (policy) and 1 (critic only) of an update of 2: the timed unit
    forms = {"per": lambda: t_per.td3_update(r_per, 2),
             "plain": lambda: t_plain.td3_update(r_plain, 2)}
    ms, issue = timed(forms, a.repeats)
    assert t_plain.per_launches == 0 and r_plain.pri is None
    # the feature's own launches, on the store as the epochs left it
    L, s, pd, n = lib(), stream_handle(), r_per.per_ref(), a.capacity
    seed = (100, 0)
    kernels = {
        "nav_per_sums": lambda: L.nav_per_sums(pd, n, s),
        "nav_per_sample": lambda: L.nav_per_sample(pd, n, B, *seed, 7, a.per_beta, ptr(t_per.idx_c),
                                                   ptr(t_per.w_per), ptr(t_per.idx_a), s),
        "nav_per_sample_critic_only": lambda: L.nav_per_sample(
            pd, n, B, *seed, 7, a.per_beta, ptr(t_per.idx_c), ptr(t_per.w_per), None, s),
        "nav_per_update": lambda: L.nav_per_update(pd, B, ptr(t_per.idx_c), ptr(t_per.td_abs1),
                                                   ptr(t_per.td_abs2), a.per_alpha, 1e-6, s),
        "nav_per_stamp_65536": lambda: L.nav_per_stamp(pd, 0, min(65536, n), s),
    }
    pri = r_per.pri.clone()  # (the stamp and update forms write the store: put it back after)
    kms, _ = timed(kernels, a.repeats)
    r_per.pri.copy_(pri)
    p = pri.cpu().numpy().view("uint32")
    res = {"batch": B, "hidden": a.hidden, "n_hidden": a.n_hidden, "capacity": a.capacity,
           "per_alpha": a.per_alpha, "per_beta": a.per_beta,
           "per_launches_per_unit": t_per.per_launches // (3 + a.repeats),
           "priorities": {"min": int(p.min()), "max": int(p.max()),
                          "distinct": int(len(set(p.tolist())))},
           **{k: summary(v) for k, v in ms.items()},
           "host_issue_ms": {k: round(statistics.median(v), 4) for k, v in issue.items()},
           "kernels": {k: summary(v) for k, v in kms.items()}}
    res["per_over_plain"] = round(res["per"]["median_ms"] / res["plain"]["median_ms"], 4)
    res["added_ms"] = round(res["per"]["median_ms"] - res["plain"]["median_ms"], 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"Prioritised replay: one policy epoch + one critic-only epoch, {a.hidden} x "
                    f"{a.n_hidden}, batch {B}, ring {a.capacity} rows full, one MI355X; medians "
                    f"of {a.repeats}, the forms interleaved in one process "
                    "(tools/per_bench.py).\n\n")
            for k in ("per", "plain"):
                v = res[k]
                f.write(f"  {k:<6} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f}); host issue {res['host_issue_ms'][k]:.4f} ms\n")
            f.write(f"  per / plain {res['per_over_plain']:.4f}, added {res['added_ms']:.4f} ms "
                    f"per unit ({res['per_launches_per_unit']} nav_per_* calls)\n\n"
                    "Each nav_per_* entry point alone (event time around one call):\n")
            for k, v in res["kernels"].items():
                f.write(f"  {k:<28} median {v['median_ms']:.4f} ms  (min {v['min_ms']:.4f}, max "
                        f"{v['max_ms']:.4f})\n")
            f.write("\n" + json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
