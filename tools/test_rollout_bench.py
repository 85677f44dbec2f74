"""Time of a vectorised test episode: the fused launch against the loop it replaces.

In one process, per size (65 536 and 4 096 envs, hidden 256 x 2, a freshly initialised actor):
  (a) nav_test_rollout, max_steps steps in one launch;
  (b) the unfused loop: per step nav_act(mode=1) then nav_env_step on a scratch env (two launches
      per step, no host masking), which is all the library offered before.
Both with goal_threshold = 0 (no env ever stops), so they do the same work; one more run of (a)
with the default threshold shows what early exit is worth on that policy. HIP-event times after a
warm-up of every shape, (a) and (b) alternating, --repeats each; per leg the median, min and max,
and the spread (max - min) / median the comparison has to beat.

python tools/test_rollout_bench.py [--max-steps 200] [--repeats 7]
                                   [--out profiles/test_rollout_bench.json]
"""
import argparse
import ctypes as C
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
            "spread": round((max(ms) - min(ms)) / med, 4), "runs": len(ms)}


def bench_size(n, hidden, n_hidden, max_steps, repeats, seed):
    from nav._lib import lib, ptr, stream_handle
    from nav.fields import make_field_device
    from nav.mlp import DeviceMLP
    from nav.vec_env import VecEnv
    dev = torch.device("cuda")
    field = make_field_device(seed, dev)
    actor = DeviceMLP(2, 2, hidden, n_hidden, dev).init_kaiming(torch.Generator().manual_seed(seed))
    env0 = VecEnv(n, field, seed=seed, demo_flag=False, device=dev, goal_threshold=0.0)
    env5 = VecEnv(n, field, seed=seed, demo_flag=False, device=dev)  # default threshold
    start = env0.state.clone()  # the first reset's states
    scratch = VecEnv(n, field, seed=seed, device=dev, init=False, goal_threshold=0.0)
    scratch.goal.copy_(env0.goal)
    action = torch.zeros(n, 2, dtype=torch.float64, device=dev)
    d = actor.desc()
    L, st = lib(), stream_handle()

    def fused():
        env0.test_rollout(actor, max_steps, start=start)

    def fused_exit():
        env5.test_rollout(actor, max_steps, start=start)

    def unfused():
        for _ in range(max_steps):
            L.nav_act(C.byref(scratch.p), C.byref(d), n, ptr(scratch.state), ptr(scratch.goal),
                      None, None, 0, 1, ptr(action), None, st)
            L.nav_env_step(C.byref(scratch.p), C.byref(scratch.soa), ptr(field), ptr(action),
                           None, st)

    def run_unfused():
        scratch.state.copy_(start)
        torch.cuda.synchronize()
        return timed(unfused)

    # warm-up: every shape once, then the same results from both legs
    run_unfused()
    fused()
    fused_exit()
    torch.cuda.synchronize()
    same = bool(torch.equal(env0.test_rollout(actor, max_steps, start=start)["final_state"],
                            scratch.state))
    a, b, c = [], [], []
    for _ in range(repeats):
        a.append(timed(fused))
        b.append(run_unfused())
        c.append(timed(fused_exit))
    out5 = env5.test_rollout(actor, max_steps, start=start)
    ra, rb = summary(a), summary(b)
    return {"n_envs": n, "hidden": hidden, "n_hidden": n_hidden, "max_steps": max_steps,
            "fused": ra, "unfused": rb, "fused_default_threshold": summary(c),
            "reached_default_threshold": int(out5["reached"].sum().item()),
            "final_states_equal": same,
            "unfused_over_fused": round(rb["median_ms"] / ra["median_ms"], 3),
            "fused_us_per_step": round(1e3 * ra["median_ms"] / max_steps, 3),
            "unfused_us_per_step": round(1e3 * rb["median_ms"] / max_steps, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1707366464)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from nav._lib import require_gpu
    require_gpu()
    assert args.repeats >= 5
    res = {"device": torch.cuda.get_device_name(0),
           "sizes": [bench_size(n, args.hidden, args.n_hidden, args.max_steps, args.repeats,
                                args.seed) for n in args.sizes]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
