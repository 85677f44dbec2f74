"""The cost of learning from demonstrations (tuning only, not a test).

python tools/actor_rows_bc_bench.py [--batch 32768 --hidden 256 --layers 2 --b-demo 8192
                                     --reps 200 --runs 5 --trainer-steps 60]

In one process, with HIP events on the launch stream:
- nav_td3_actor_rows (plain) against nav_td3_actor_rows_bc (the TD3_BC form) on the same
  injected indices, `runs` alternating runs of `reps` launches each;
- in the same alternation nav_td3_actor_rows_bcq (the Q-filtered BC form, the critic's forward on
  (s, a_demo) inside the launch) and what it replaces, three launches: a gather of the B_demo
  demonstration rows, nav_mlp_forward of critic 1 on them, then the BC form;
- nav_td3_mix_idx at the same batch;
- ms per VecTrainer.step() with demo_fraction 0.25 / bc_weight 1 against the default trainer,
  alternating (n_envs = 2 * batch as bench.py's flagship shape), when --trainer-steps > 0.
Prints one JSON line: every run's figure, the medians and the ranges.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "residual-td3-robot-navigation_amd"))

import torch  # noqa: E402


def timeit(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def summary(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3),
            "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--b-demo", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trainer-steps", type=int, default=60)
    args = ap.parse_args()
    from nav._lib import NavReplay, lib, ptr, require_gpu, stream_handle
    from nav.mlp import DeviceMLP
    require_gpu()
    dev, H, nh, B, bd = "cuda", args.hidden, args.layers, args.batch, args.b_demo
    g = torch.Generator().manual_seed(0)
    actor = DeviceMLP(2, 2, H, nh, dev).init_kaiming(g)
    critic = DeviceMLP(4, 1, H, nh, dev).init_kaiming(g)
    hp, L, s = actor.hp, lib(), stream_handle()
    cap, n_tail = 4 * B, 3 * 199 * 64
    rows = (torch.rand(cap + n_tail, 8, device=dev) * 99).contiguous()
    rd = NavReplay(rows.data_ptr(), cap)
    idx_c = torch.zeros(B, dtype=torch.int64, device=dev)
    idx_a = torch.zeros(B, dtype=torch.int64, device=dev)

    def mix():
        L.nav_td3_mix_idx(cap, B, bd, cap, n_tail, 1, 2, 3, ptr(idx_c), ptr(idx_a), s)
    mix()
    f = lambda *sh: torch.zeros(*sh, device=dev)  # noqa: E731
    nblk = L.nav_mlp_row_blocks(B)
    mid = actor.middle_layers()
    batch, q, da, part = f(B, 8), f(B), f(B, 2), f(nblk)
    acts, dz = f(nh, B, hp), f(nh, B, hp)
    ma, mc = actor.mask_buffer(B), critic.mask_buffer(B)
    es = f(nblk, L.nav_mlp_edge_count(2, 2, hp, nh))
    ad, cd = actor.desc(), critic.desc()
    head = (C.byref(ad), C.byref(cd), C.byref(rd), cap, B, ptr(idx_a), 1, 2, 3)
    tail = (ptr(acts), mid, ptr(dz), mid, ptr(ma), ptr(mc), ptr(es), s)

    def plain():
        L.nav_td3_actor_rows(*head, ptr(batch), ptr(q), ptr(da), *tail)

    def bc():
        L.nav_td3_actor_rows_bc(*head, bd, 1.0, 1.0, ptr(batch), ptr(q), ptr(da), ptr(part),
                                *tail)
    q_demo, keep = f(B), torch.zeros(nblk, dtype=torch.int32, device=dev)

    def bcq():
        L.nav_td3_actor_rows_bcq(*head, bd, 1.0, 1.0, ptr(batch), ptr(q), ptr(da), ptr(part),
                                 ptr(q_demo), ptr(keep), *tail)
    # the unfused alternative: gather, critic forward on the gathered rows, the BC form
    gathered, q_alt, demo_idx = f(bd, 8), f(bd), idx_a[:bd]
    out1 = (C.c_void_p * 1)(q_alt.data_ptr())

    def two_launch():
        torch.index_select(rows, 0, demo_idx, out=gathered)
        L.nav_mlp_forward(C.byref(cd), 1, bd, ptr(gathered), 8, 0, out1, 1, 0, 0, None, 0.0, 0.0,
                          0.0, 0, 0, 0, None, 0, None, s)
        bc()
    t_plain, t_bc, t_bcq, t_two, t_mix = [], [], [], [], []
    for _ in range(args.runs):
        t_plain.append(timeit(plain, args.reps))
        t_bc.append(timeit(bc, args.reps))
        t_bcq.append(timeit(bcq, args.reps))
        t_two.append(timeit(two_launch, args.reps))
        t_mix.append(timeit(mix, args.reps))
    torch.cuda.synchronize()
    res = {"batch": B, "hidden": H, "layers": nh, "b_demo": bd, "reps": args.reps,
           "actor_rows_us": summary(t_plain), "actor_rows_bc_us": summary(t_bc),
           "actor_rows_bcq_us": summary(t_bcq), "gather_forward_bc_us": summary(t_two),
           "bcq_kept_fraction": round(keep.sum().item() / bd, 4),
           "mix_idx_us": summary(t_mix)}
    if args.trainer_steps > 0:
        from nav.trainer import VecTrainer
        kw = dict(n_envs=2 * B, hidden=H, n_hidden=nh, batch=B, updates_per_step=2, device=dev)
        trs = {"default": VecTrainer(**kw),
               "demos": VecTrainer(demo_fraction=0.25, bc_weight=1.0, **kw)}
        for tr in trs.values():
            for _ in range(10):
                tr.step()
        torch.cuda.synchronize()
        ms = {k: [] for k in trs}
        for _ in range(args.runs):
            for k, tr in trs.items():
                t0 = time.perf_counter()
                for _ in range(args.trainer_steps):
                    tr.step()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.trainer_steps)
        res["ms_per_step"] = {k: summary(v) for k, v in ms.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
