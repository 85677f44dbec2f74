#!/usr/bin/env python3
"""bench.py — env-steps/s of the vectorised residual-TD3 loop on MI355X (BASELINE.json metric).

Workload (BASELINE.json config 3): 65 536 parallel envs per GPU, full residual-TD3 update with
2 x 256 actor/critic MLPs. One bench step = one vector tick of every env (nav_act_tick: actor
forward + tick + indexed demo reward in one launch) followed by `--updates` TD3 epochs (critic
every epoch, actor + Polyak every 2nd) at batch `--batch` sampled from the device replay ring. Synthetic seeded start/goal pairs
(Philox, 64 tasks of 1 024 envs), synthetic Perlin-style fields, per-task demonstration sets from
the batched GPU CEM demonstrator (3 demos + augmentations each, as the reference's robot builds
them), random-init networks (no datasets or checkpoints exist offline).

N > 1 (torch.distributed.run, one process per GPU): independent env blocks per rank (seed +
rank), no data-path collective ("scaling": "weak"); `--shared-policy` adds the RCCL all-reduce of
flat actor/critic gradients (BASELINE config 5). Rank 0 prints one JSON line.

A plain run sets up, warms up, times `--steps` steps (no HIP events inside the timed region),
writes the last timed step's results when `--dump-outputs DIR` is given, and prints the line with
`value` and `ms_per_step`. Everything else is behind `--full`: the per-kernel breakdown pass,
`roofline` for the dominant kernel (HIP-event timed inside the timed region on the launch
stream), the longer event-free run (`timed_long`), the step kernel's HBM figure on a large-N
sweep (`step_kernel`, the 2^24-env point), the per-tick time at 65 536 envs in both launch forms
(`tick_forms`: nav_act + nav_agent_step_indexed vs the fused nav_act_tick), the update-to-data
sweep, and `cpu_baseline` (the oracle CPU port of the same loop, rank 0 only, bounded sample).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "residual-td3-robot-navigation_amd"))

import torch  # noqa: E402

from nav import prof  # noqa: E402

EVENT_SAMPLE = 8             # timed region: event pairs around 1 launch in 8 of the dominant kernel
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_VALU_PEAK_TFS = 78.6    # MI355X spec FP64 vector
F16_MFMA_PEAK_TFS = 2516.6  # MI355X_MICROARCH.md: 1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz
#                             (dense fp16 = bf16 rate)
# The row kernels' hidden x hidden f32 GEMMs run on the fp16 matrix cores as 3 products of a
# scaled two-plane split (lo.hi + hi.lo + hi.hi; rounds 3-4: 6 products of a three-plane bf16
# split); since round 6 the top layer's row backward of the d_out = 1 critics takes 2 (its A
# operand is the forward's ReLU bit, exact in fp16: gemm_bits)
PRODUCTS_PER_PASS = 3
PRODUCTS_BITS = 2


def products_per_f32(region):
    """fp16 MFMA products per f32 product of the weight-gradient kernels: 3, except the factored
    critic weight gradient k_wgrad_fact, whose A operand (the ReLU bit) is exact in fp16: 2."""
    return 2 if region == "mlp_wgrad_fact" else PRODUCTS_PER_PASS


def layer_products(region, rows, layers):
    """fp16 products x hidden-layer GEMMs one row block of the region's kernel runs (each such
    GEMM is 2 x rows x hp^2 FLOP per product). A forward pass: (layers - 1) hidden GEMMs at 3; a
    critic (d_out = 1) row backward: its top layer at 2 (gemm_bits) + the rest at 3; the actor's
    row backward (d_out = 2): all at 3. critic_rows: target actor + 2 target critics + 2 online
    forwards + 2 critic backwards (at batches <= 2048 the twins split into two workgroups that
    each repeat the 3 target passes); actor_rows: actor + critic forwards, critic backward, actor
    backward; the acting forward / tick: one forward."""
    h = layers - 1
    fwd = 3 * h
    cbwd = (PRODUCTS_BITS + 3 * (h - 1)) if h >= 1 else 0
    if region == "critic_rows":
        return (8 if rows <= 2048 else 5) * fwd + 2 * cbwd
    if region == "actor_rows":
        return 2 * fwd + cbwd + 3 * h
    return fwd if region in ("act", "act_tick") else 0


# the median shader clock each row kernel holds under the bench loop (tools/clock_probe.py)
HELD_CLOCK_MHZ = {"critic_rows": 1925.3, "actor_rows": 1964.5, "act_tick": 2048.1}
ROOFLINE_VERSION = ("r06: fp16 two-plane split, 3 products per f32 product, 2 in the critics' "
                    "top-layer row backward (r05: 3 everywhere; r03-r04: bf16 6)")


# what the path computes in: the hidden x hidden GEMMs are NOT fp32 MFMA but fp16 MFMA products
# of a scaled two-plane split of each f32 operand (22 significant bits, lo.lo dropped), f32
# accumulate; the thin layers, epilogues, losses and Adam in f32; the env state in f64
DTYPE = ("f32-accurate MLP: fp16x2 split (22-bit operands) on fp16 MFMA, f32 accumulate; "
         "f32 edge layers / losses / Adam; fp64 env state")
ACCURACY = {"hidden_gemm_err_vs_fp64": "2.4e-7 .. 5.7e-7 of max|ref| (fp32 itself ~1e-7)",
            "wgrad_err_vs_fp64": "1.7e-7 .. 8.1e-7 of scale",
            "bound_tested": "2e-6 of max|ref|",
            "test": "tests/test_gpu_mlp.py::test_split_gemm_f32_accuracy_vs_fp64",
            "source": "profiles/r05i_accuracy.log"}
# SURVEY 8(d)'s graded bytes per env-step: fused step + reward + done + stuck 105 B, the pure
# Environment.step 24 B (f32 state, no replay row; this build keeps f64 state and writes a 32-B
# replay row: 237 B / 48 B in its own accounting, prof.AGENT_STEP_BYTES / ENV_STEP_BYTES)
GRADED_AGENT_STEP_BYTES = 105
GRADED_ENV_STEP_BYTES = 24


def graded_step_fracs(sweep):
    """HBM fraction of the step kernels in SURVEY 8(d)'s byte accounting, from the sweep's event
    times: per sweep size, agent_step at 105 B and env_step at 24 B per env-step."""
    out = []
    for row in sweep:
        n = row["n_envs"]
        e = {"n_envs": n}
        for k, b in (("agent_step", GRADED_AGENT_STEP_BYTES), ("env_step", GRADED_ENV_STEP_BYTES)):
            gbs = b * n / (row[k]["avg_us"] * 1e-6) / 1e9
            e[k] = {"bytes_per_env_step": b, "GBps": round(gbs, 1),
                    "frac": round(gbs / HBM_PEAK_GBS, 4)}
        out.append(e)
    return out


# HBM bytes per launch from the committed rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this same
# command (tools/pmc_traffic.py, gfx950 correction applied); bench regions -> kernel names
PMC_TRAFFIC = os.path.join(HERE, "profiles", "pmc_traffic.json")
REGION_KERNEL = {"critic_rows": "k_td3_critic_rows", "actor_rows": "k_td3_actor_rows",
                 "mlp_bwd": "k_mlp_bwd", "mlp_wgrad": "k_wgrad",
                 "mlp_wgrad_fact": "k_wgrad_fact", "act": "k_mlp_fwd",
                 "agent_step": "k_agent_step", "env_step": "k_env_step",
                 "act_tick": "k_mlp_fwd<tick>", "env_step_k": "k_env_step_k",
                 "grad_reduce": "k_grad_reduce", "demo_reward": "k_demo_reward_idx"}


def pmc_traffic(region):
    """(bytes per launch, source) of the region's kernel from the committed PMC summary, else
    (None, None). bytes per launch = WRITE_SIZE + FETCH_SIZE, the fetch doubled only for the
    streaming kernels (tools/pmc_traffic.py); the source string carries the raw figure too."""
    try:
        with open(PMC_TRAFFIC) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, None
    k = t.get(REGION_KERNEL.get(region, ""))
    if not k:
        return None, None
    return k["bytes_per_launch"], "profiles/pmc_traffic.json (%s; raw %s B, fetch x%s)" % (
        t["_meta"].get("command", ""), k.get("bytes_raw"), k.get("fetch_correction", 2.0))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--envs-per-group", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1707366464)
    ap.add_argument("--shared-policy", action="store_true")
    # shared policy: the next collect on a second stream beside the last epoch's all-reduce
    ap.add_argument("--overlap-collect", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also the per-kernel breakdown, the roofline of the dominant kernel "
                         "(HIP events inside the timed region), timed_long, tick_forms, the "
                         "step-kernel sweep, the update-to-data sweep and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as "
                         "DIR/<name>.npy (float32 / float64)")
    # the --no-* switches and --long-steps trim a --full run; a plain run has none of these legs
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-utd-sweep", action="store_true")
    ap.add_argument("--long-steps", type=int, default=200,
                    help="extra event-free timed run of this many steps (extra key timed_long)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--breakdown", action="store_true", help="print the per-kernel table")
    ap.add_argument("--presleep", type=int, default=0,
                    help="diagnostic: a GPU sleep of this many cycles before the timed loop, so "
                         "the host queues ahead (launch-gap check under rocprofv3)")
    ap.add_argument("--no-timed-events", action="store_true",
                    help="no HIP events inside the timed region (overhead check; no roofline)")
    ap.add_argument("--sweep-only", type=int, default=0,
                    help="only run the step-kernel sweep at this N (profiling helper)")
    ap.add_argument("--launch-check", action="store_true",
                    help="test helper: only the rank launch + gloo rendezvous, no GPU")
    return ap.parse_args()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args, argv):
    """`bench.py --gpus N` (N > 1) without an outer torch.distributed.run: start one as a CHILD
    process (never exec: this parent may not replace itself), one rank per GPU, each rank this
    same script with the same arguments. The ranks inherit stdout, so rank 0's single JSON line is
    this command's output; the exit code is the launcher's, non-zero when any rank fails. Nothing
    here touches the GPU (device_count does not initialise it on this image)."""
    import subprocess
    n = args.gpus
    if not args.launch_check and os.environ.get("NAV_DIST_REHEARSAL") != "1":
        have = torch.cuda.device_count()
        if have < n:
            print(f"bench.py: --gpus {n} but {have} GPU(s) visible", file=sys.stderr, flush=True)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={n}", "--master-addr=127.0.0.1",
           f"--master-port={_free_port()}", os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts
    return subprocess.run(cmd, env=env).returncode


def launch_check(ws, rank):
    """--launch-check: the N > 1 launch path without a GPU (CPU test): each rank joins a gloo
    group, the ranks' ids are summed, rank 0 prints one JSON line with n_gpus = world size."""
    import torch.distributed as dist
    if ws > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    t = torch.tensor([float(rank)])
    if ws > 1:
        dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": ws, "rank_sum": int(t.item())}),
              flush=True)
    if ws > 1:
        dist.destroy_process_group()


def dist_setup(args):
    """One process per GPU over RCCL ("nccl"). NAV_DIST_REHEARSAL=1 (rehearsal of the N > 1
    code path on a one-GPU box only): every rank on cuda:0 and gloo collectives, since RCCL refuses
    two ranks on one device; the timing of such a run means nothing."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if ws > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("NAV_DIST_REHEARSAL") == "1":
            local = 0
            torch.cuda.set_device(0)
            torch.distributed.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    return ws, rank, local


def barrier(ws):
    if ws > 1:
        torch.distributed.barrier()


def step_kernel_sweep(field, sizes, reps=20, K=16):
    """Step-kernel HBM figure: nav_agent_step (fused tick), nav_env_step (pure
    Environment.step) and nav_env_step_k (K Environment.steps per launch, state in registers)
    alone at growing N; per-env-step figures. Each kernel runs `reps` times back to back between
    one event pair on the launch stream (avg = span / reps): per-launch event pairs add a fixed
    ~4-6 us at 65 536 envs, where the kernels themselves run 4-7 us (kernel trace,
    profiles/r02r_sweep_65536_kernel_trace.txt)."""
    from nav.vec_env import ReplayRing, VecEnv
    out = []
    for n in sizes:
        env = VecEnv(n, field, seed=11, envs_per_group=n, demo_flag=False)
        rep = ReplayRing(n, "cuda")
        act = (torch.rand(n, 2, dtype=torch.float64, device="cuda") - 0.5) * 14
        acts = (torch.rand(K, n, 2, dtype=torch.float64, device="cuda") - 0.5) * 14
        for _ in range(6):  # fill the 5-deep stuck history: steady-state traffic
            env.agent_step(act, rep)
            env.step(act)
        env.step_k(acts)
        row = {"n_envs": n}
        # each kernel back to back, as a training loop / a pure Environment.step loop runs it
        # (interleaved, env_step paid the write-back of agent_step's dirty lines: PMC r01p)
        for k, bpe, steps, fn, r in (
                ("agent_step", prof.AGENT_STEP_BYTES, 1, lambda: env.agent_step(act, rep), reps),
                ("env_step", prof.ENV_STEP_BYTES, 1, lambda: env.step(act), reps),
                ("env_step_k", prof.env_step_k_bytes(K, False), K, lambda: env.step_k(acts),
                 max(2, reps // 4))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(r):
                fn()
            e1.record()
            e1.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / r
            row[k] = {"avg_us": round(us, 2), "env_steps_per_launch": steps,
                      "bytes_per_env_step": bpe,
                      "GBps": round(bpe * n * steps / (us * 1e-6) / 1e9, 1),
                      "env_steps_per_s": n * steps / (us * 1e-6)}
        out.append(row)
        del env, rep, act, acts
        torch.cuda.empty_cache()
    return out


def tick_forms(tr, reps=50):
    """Per-tick time of the collect half of a step at the trainer's env count, in both launch
    forms: nav_act + nav_agent_step_indexed (two launches) and nav_act_tick (one), HIP events on
    the launch stream. Runs the trainer's own envs (after the timed regions)."""
    from nav import prof
    fuse = tr.fuse_tick
    res = {"n_envs": tr.n}
    for form in ("two_launch", "fused"):
        tr.fuse_tick = form == "fused"
        t = prof.KernelTimer(["act", "agent_step", "act_tick"])
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        with prof.timing(t):
            for _ in range(reps):
                tr.collect()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) / reps
        s = t.summary()
        ks = ("act", "agent_step") if form == "two_launch" else ("act_tick",)
        res[form] = {k: round(s[k]["avg_us"], 2) for k in ks}
        res[form]["per_tick_us"] = round(sum(s[k]["avg_us"] for k in ks), 2)
        res[form]["wall_per_tick_us"] = round(1e6 * wall, 2)
    tr.fuse_tick = fuse
    return res


def cpu_info():
    """(CPU model, CPUs this process may run on, CPUs the machine has). os.cpu_count() ignores
    the lease's affinity mask; sched_getaffinity does not."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, len(os.sched_getaffinity(0)), os.cpu_count()


def cpu_baseline(args, trainer):
    """The oracle CPU port of the same workload (C OpenMP tick with the same exact demo index as
    the GPU, torch-CPU fp32 TD3), bounded sample; plus the single-env one-core C rates."""
    from oracle.cpu_loop import CPUPort, single_env_rates, time_port
    from oracle import oracle as O
    n = args.envs
    fields = trainer.field.cpu().numpy()
    speed, angle = fields[..., 0].copy(), fields[..., 1].copy()
    pts = trainer.env.demo_xy.cpu().numpy()
    off = trainer.env.demo_off.cpu().numpy() if trainer.env.demo_off is not None else \
        [0, len(pts)]
    model, affinity, machine = cpu_info()
    # one thread per CPU this process may use, capped by the lease's CPU share (OMP_NUM_THREADS,
    # 16 per GPU on the box): the OpenMP env tick and torch's intra-op pool both run that many
    share = int(os.environ.get("OMP_NUM_THREADS", affinity) or affinity)
    threads = max(1, min(affinity, share))
    O.lib().orc_set_threads(threads)
    torch_threads = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        port = CPUPort(n, args.hidden, args.layers, args.batch, args.updates,
                       args.envs_per_group, args.seed, speed, angle, pts, off)
        k, dt = time_port(port, args.cpu_budget, 64)
        omp = O.lib().orc_threads()
        used = torch.get_num_threads()
    finally:
        torch.set_num_threads(torch_threads)
    single = single_env_rates(speed, angle, pts[off[0]:off[1]], 2.0)
    return {"value": k * n / dt, "unit": "env-steps/s", "cores": threads,
            "kind": "port",
            "sample": f"{k} vector steps of the same workload ({n} envs, TD3 {args.updates} "
                      f"epochs x batch {args.batch}, {args.layers}x{args.hidden}) on the oracle "
                      f"CPU port: C OpenMP env tick with the same exact bucketed demo index as the "
                      f"GPU + torch-CPU fp32 TD3, {threads} threads, {dt:.1f} s",
            "cpu_model": model, "affinity_cpus": affinity, "omp_threads": omp,
            "torch_threads": used, "cpu_share": share, "machine_cpus": machine,
            "cores_note": "cores = threads run = min(CPUs in this process's affinity mask, the "
                          "lease's CPU share OMP_NUM_THREADS); machine_cpus is os.cpu_count(), "
                          "which ignores the affinity mask",
            "single_env_1core": {k2: round(v, 1) for k2, v in single.items()},
            "single_env_note": "one env, one core, the C restatement looping in one call: "
                               "Environment.step alone / the whole agent tick without the learner"}


def timed_steps(tr, steps, ws, dev):
    """Wall time of `steps` training steps between barrier + synchronize on both sides, max over
    ranks."""
    from nav.dist import max_over_ranks
    barrier(ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    barrier(ws)
    dt = time.perf_counter() - t0
    return max_over_ranks(dt, dev) if ws > 1 else dt


def utd_sweep(args, dev, points=((8192, 2), (32768, 2), (32768, 8)), steps=30):
    """env-steps/s at other update-to-data ratios (sampled transitions per collected one =
    epochs x batch / envs): 0.25, 1 (the headline's), 4."""
    from nav.trainer import VecTrainer
    out = []
    for batch, epochs in points:
        tr = VecTrainer(n_envs=args.envs, hidden=args.hidden, n_hidden=args.layers, batch=batch,
                        updates_per_step=epochs, seed=args.seed,
                        envs_per_group=args.envs_per_group, device=dev)
        for _ in range(4):
            tr.step()
        dt = timed_steps(tr, steps, 1, dev)
        out.append({"update_to_data": epochs * batch / args.envs, "batch": batch,
                    "td3_epochs_per_step": epochs, "steps": steps,
                    "ms_per_step": round(1e3 * dt / steps, 4),
                    "env_steps_per_s": args.envs * steps / dt})
        del tr
        torch.cuda.empty_cache()
    return out


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def step_outputs(tr):
    """What one VecTrainer.step() leaves for its caller, by name: the actions the actor chose, the
    tick's results (next_state, goal_term, flags), the per-env state after the auto-reset, the
    replay rows this step pushed (in env order) and the parameters of the six networks after the
    learner's epochs."""
    env, rep = tr.env, tr.replay
    out = {"action": tr.action, "next_state": env.next_state, "goal_term": env.goal_term,
           "flags": env.flags}
    for k in tr.ENV_STATE:
        out["env_" + k] = getattr(env, k)
    slots = (rep.position - tr.n + torch.arange(tr.n, device=rep.rows.device)) % rep.capacity
    out["replay_rows"] = rep.rows[slots]
    for k, net in tr.td3.networks().items():
        out["net_" + k] = net.params
    return out


def dump_outputs(tr, path):
    """--dump-outputs: step_outputs() as DIR/<name>.npy, float32 tensors as they are and every
    other dtype as float64 (exact for the integer state). Whole arrays while they fit 64 MB in all
    (16.9 MB at the default sizes); past that, an array over its equal share of the budget is
    written as a fixed seeded sample of its flattened entries."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    torch.cuda.synchronize()
    arrays = {}
    for k, t in step_outputs(tr).items():
        a = t.detach().cpu().numpy()
        arrays[k] = a if a.dtype == np.float32 else a.astype(np.float64)
    share = DUMP_BUDGET_BYTES // len(arrays)
    fits = sum(a.nbytes for a in arrays.values()) <= DUMP_BUDGET_BYTES
    for i, (k, a) in enumerate(sorted(arrays.items())):
        if not fits and a.nbytes > share:
            keep = share // a.itemsize
            ix = np.sort(np.random.default_rng(i).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[ix]
        np.save(os.path.join(path, k + ".npy"), a)


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            return launch_ranks(args, sys.argv[1:])
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        print(f"bench.py: WORLD_SIZE={os.environ['WORLD_SIZE']} but --gpus {args.gpus}",
              file=sys.stderr, flush=True)
        return 2
    if args.launch_check:
        return launch_check(int(os.environ.get("WORLD_SIZE", "1")),
                            int(os.environ.get("RANK", "0")))
    ws, rank, local = dist_setup(args)
    from nav import prof
    from nav._lib import lib, require_gpu
    from nav.trainer import VecTrainer
    require_gpu()
    lib()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.sweep_only:
        from nav.fields import make_fields
        from nav.vec_env import make_field
        print(json.dumps(step_kernel_sweep(make_field(*make_fields(args.seed), dev),
                                           [args.sweep_only])), flush=True)
        return
    from nav.dist import broadcast_params, make_grad_hook, max_over_ranks, shard_seed
    hook = make_grad_hook(ws) if args.shared_policy else None  # RCCL all-reduce over xGMI
    # shared policy: the global batch is split over the ranks (each samples B / world rows from
    # its local replay, the SUM all-reduce + / world makes it the full-batch update)
    rank_batch = args.batch // ws if (args.shared_policy and ws > 1) else args.batch
    tr = VecTrainer(n_envs=args.envs, hidden=args.hidden, n_hidden=args.layers, batch=rank_batch,
                    updates_per_step=args.updates, seed=shard_seed(args.seed, rank),
                    envs_per_group=args.envs_per_group, device=dev, grad_hook=hook,
                    overlap_collect=args.overlap_collect and hook is not None)
    if args.shared_policy and ws > 1:  # same initial policy on every rank
        nets = list(tr.td3.networks().values())
        broadcast_params([n.params for n in nets])
        for n in nets:
            n.pack()
    # warmup: first step fills the replay ring past one batch; then breakdown pass
    for _ in range(max(args.warmup, 1)):
        tr.step()
    torch.cuda.synchronize()
    tracked = []
    if args.full:
        bd = prof.KernelTimer()
        with prof.timing(bd):
            for _ in range(2):
                tr.step()
        breakdown = bd.summary()
        # the dominant KERNEL (the all-reduce region is a collective, reported apart)
        dominant = max((k for k in breakdown if k != "allreduce"),
                       key=lambda k: breakdown[k]["total_ms"])
        tracked = [dominant] + (["allreduce"] if hook is not None else [])

    # ---- timed region
    # --full: the dominant kernel's launches are bracketed by HIP event pairs on its launch
    # stream, one launch in EVENT_SAMPLE (each record stalls the stream a few us; bracketing
    # every launch cost 2.6 % of the step, profiles/r03c_bench.json value vs timed_long); with a
    # shared policy the all-reduce messages are sampled the same way. A plain run (and
    # --no-timed-events) records no event: the timer tracks no region
    timer = prof.KernelTimer([] if args.no_timed_events else tracked,
                             sample_every=EVENT_SAMPLE)
    barrier(ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.presleep:
        torch.cuda._sleep(args.presleep)
    with prof.timing(timer):
        for _ in range(args.steps):
            tr.step()
    torch.cuda.synchronize()
    barrier(ws)
    dt = time.perf_counter() - t0
    if ws > 1:
        dt = max_over_ranks(dt, dev)
    ksum = timer.summary()
    env_steps = args.envs * args.steps * ws
    value = env_steps / dt
    if args.dump_outputs:  # the last timed step's results, before any further step runs
        dump_outputs(tr, args.dump_outputs if rank == 0 else
                     os.path.join(args.dump_outputs, "rank%d" % rank))
    head = {
        "metric": "env-steps/sec at 65 536 parallel envs (full residual-TD3 update)",
        "value": value, "unit": "env-steps/s", "n_gpus": ws, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE,
        "accuracy": ACCURACY,
        "data": "synthetic (Philox start/goal pairs, generated fields, batched-CEM demo sets)",
        "config": {"workload": "config3: 65536 envs + residual-TD3 (2x256 MLPs)",
                   "envs_per_gpu": args.envs, "envs_per_group": args.envs_per_group,
                   "hidden": args.hidden, "layers": args.layers, "batch": args.batch,
                   "td3_epochs_per_step": args.updates,
                   "rank_batch": rank_batch,
                   "update_to_data": args.updates * args.batch / args.envs,
                   "parallelism": ("dp%d-shared-policy%s" % (
                                       ws, "-overlap-collect" if tr.overlap_collect else "")
                                   if args.shared_policy and ws > 1
                                   else "independent-env-blocks x%d" % ws)},
        "full": args.full,
    }
    # a longer event-free timed run beside the contract's K steps (extra key)
    timed_long = None
    if args.full and args.long_steps > 0:
        dtl = timed_steps(tr, args.long_steps, ws, dev)
        timed_long = {"steps": args.long_steps, "ms_per_step": 1e3 * dtl / args.long_steps,
                      "value": args.envs * args.long_steps * ws / dtl,
                      "note": "same loop, no HIP events in the timed region"}

    if rank == 0 and args.no_timed_events:
        print(json.dumps({"value": value, "ms_per_step": 1e3 * dt / args.steps,
                          "no_timed_events": True}), flush=True)
    elif rank == 0 and not args.full:
        print(json.dumps(head), flush=True)
    elif rank == 0:
        d = ksum[dominant]
        traffic, traffic_src = pmc_traffic(dominant)
        is_bytes = dominant in ("agent_step", "env_step", "grad_reduce")
        ach = d["work_per_launch"] / (d["avg_us"] * 1e-6)
        if is_bytes:
            roof = {"bound": "hbm", "kernel": dominant, "achieved": round(ach / 1e9, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic,
                    "traffic_source": traffic_src}
        elif dominant == "demo_reward":
            tf = ach / 1e12
            roof = {"bound": "valu", "kernel": dominant, "achieved": round(tf, 2),
                    "peak": FP64_VALU_PEAK_TFS, "unit": "TFLOP/s",
                    "frac": round(tf / FP64_VALU_PEAK_TFS, 4), "traffic": traffic,
                    "traffic_source": traffic_src, "avg_us": round(d["avg_us"], 2)}
        else:
            # the matrix-core view: the MFMA FLOPs the kernel's hidden x hidden GEMMs execute
            # (each f32 product as 3 fp16 products of the scaled two-plane split) against the
            # fp16 dense peak; the f32-equivalent rate of all its FLOPs is a separate key
            hp = (args.hidden + 31) // 32 * 32
            rows = args.envs if dominant in ("act", "act_tick") else rank_batch
            if dominant in ("mlp_wgrad", "mlp_wgrad_fact"):
                # the weight-gradient regions carry their hidden x hidden f32 FLOPs as work
                hidden = d["work_per_launch"]
                products = products_per_f32(dominant)
                mfma_flop = products * hidden
            else:
                lp = layer_products(dominant, rows, args.layers)
                mfma_flop = lp * 2.0 * rows * hp * hp
                passes = {"critic_rows": 10 if rows <= 2048 else 7, "actor_rows": 4}
                hidden = passes.get(dominant, 1) * (args.layers - 1) * 2.0 * rows * hp * hp
                products = "3 (2 in the critics' top-layer row backward)"
            tfs = mfma_flop / (d["avg_us"] * 1e-6) / 1e12
            roof = {"bound": "mfma", "kernel": dominant, "achieved": round(tfs, 1),
                    "peak": F16_MFMA_PEAK_TFS, "unit": "TFLOP/s",
                    "frac": round(tfs / F16_MFMA_PEAK_TFS, 4),
                    "version": ROOFLINE_VERSION,
                    "fp16_products_per_f32_product": products,
                    "peak_note": "fp16 dense MFMA peak: the hidden x hidden f32 GEMMs run on the "
                                 "fp16 matrix cores as products of a power-of-two-scaled "
                                 "two-plane fp16 split (22-bit operands, f32 accumulate; pinned "
                                 "vs fp64); achieved = the MFMA FLOPs those products issue per "
                                 "launch / the launch's event-timed duration",
                    "mfma_flop_per_launch": mfma_flop,
                    "hidden_gemm_f32_flop_per_launch": hidden,
                    # DVFS: the row kernels hold ~1.93 GHz, not the 2.4 GHz of the spec peak
                    # (in-kernel s_memtime / s_memrealtime stamps, a -DNAV_CLOCK_STAMP build)
                    "held_clock": {"mhz": HELD_CLOCK_MHZ.get(dominant),
                                   "frac": (round(tfs / (F16_MFMA_PEAK_TFS *
                                                         HELD_CLOCK_MHZ[dominant] / 2400.0), 4)
                                            if dominant in HELD_CLOCK_MHZ else None),
                                   "source": "profiles/r05l_clock_probe_fp16.json (median over "
                                             "workgroups, 3 s of bench steps)"},
                    "f32_equiv": {"flop_per_launch": d["work_per_launch"],
                                  "achieved_TFs": round(ach / 1e12, 2),
                                  "note": "the kernel's algorithmic f32 FLOPs (SURVEY 8(d)) / "
                                          "launch time. NOT f32-pipe work: the hidden GEMMs "
                                          "execute on the fp16 pipe (above), so this rate may "
                                          "exceed the 157.3 TF f32 MFMA peak"},
                    "traffic": traffic, "traffic_source": traffic_src,
                    "avg_us": round(d["avg_us"], 2), "launches_timed": d["launches"],
                    "launches": timer.seen[dominant], "event_sample": EVENT_SAMPLE}
        forms = None if ws > 1 else tick_forms(tr)
        sweep = None if (args.no_sweep or ws > 1) else step_kernel_sweep(
            tr.field, [65536, 1 << 20, 1 << 22, 1 << 24])
        step_k = None
        if sweep:
            big = sweep[-1]["agent_step"]
            step_k = {"kernel": "nav_agent_step", "n_envs": sweep[-1]["n_envs"],
                      "avg_us": big["avg_us"], "bytes_per_env_step": prof.AGENT_STEP_BYTES,
                      "GBps": big["GBps"], "frac": round(big["GBps"] / HBM_PEAK_GBS, 4),
                      # SURVEY 8(d)'s graded accounting (f32 state, no replay row): the fused
                      # tick 105 B, the pure Environment.step 24 B, at 2^24 and at 65 536 envs
                      "graded": graded_step_fracs(sweep),
                      "env_step_k": sweep[-1]["env_step_k"],
                      "at_65536": sweep[0]["agent_step"]}
        # CPU baseline: rank 0 at N = 1 only (a reported baseline, not part of the scaling runs)
        cpu = None if (args.no_cpu_baseline or ws > 1) else cpu_baseline(args, tr)
        utd = None if (args.no_utd_sweep or ws > 1) else utd_sweep(args, dev)
        line = dict(
            head,
            roofline=roof,
            step_kernel=step_k,
            tick_forms=forms,
            step_kernel_sweep=sweep,
            kernels={k: {"avg_us": round(v["avg_us"], 2), "launches_per_step":
                         v["launches"] / 2, "ms_per_step": v["total_ms"] / 2}
                     for k, v in breakdown.items()},
            cpu_baseline=cpu,
            timed_long=timed_long,
            utd_sweep=utd,
        )
        if hook is not None:
            ar = ksum.get("allreduce")
            line["allreduce"] = {
                "messages_per_step": hook.calls / max(1, tr.steps),
                "bytes_per_step": hook.bytes / max(1, tr.steps),
                "backend": torch.distributed.get_backend() if ws > 1 else None,
                # event pair on the learner's stream around 1 message in EVENT_SAMPLE inside the
                # timed region (the collective's stream waits for the first event, the learner's
                # stream for the collective before the second)
                "avg_us_per_message": round(ar["avg_us"], 2) if ar else None,
                "avg_bytes_per_message": ar["work_per_launch"] if ar else None,
                "messages_timed": ar["launches"] if ar else 0,
                "ms_per_step": (ar["avg_us"] * 1e-3 * hook.calls / max(1, tr.steps)
                                if ar else None)}
        print(json.dumps(line), flush=True)
    if ws > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
