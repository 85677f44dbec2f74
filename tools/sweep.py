#!/usr/bin/env python3
"""Hyper-parameter sweep as one population (nav.population.PopulationTrainer): every configuration
trains on its own member of one env set, all members act and tick in one launch and run their test
episodes in one launch. Prints one JSON line per member: its overrides, its replica index and the
numbers of evaluate().

    python tools/sweep.py --reference-study
    python tools/sweep.py --axis demo_factor=10,30,50,70 --replicas 2 --envs-per-member 4096 \\
        --train-steps 200
    python tools/sweep.py --axis initial_noise=1,0.5 --axis noise_decay=0.5,0.75,0.9 --replicas 3
    python tools/sweep.py --reference-study --replicas 2 --pbt-every 50 \\
        --pbt-explore demo_factor=1:100 --pbt-explore critic_lr=1e-5:1e-2
    python tools/sweep.py --axis demo_reset_prob=0,0.25,0.5 --pbt-every 50 \\
        --pbt-explore demo_reset_prob=0:1

--reference-study runs the four DEMO_PROXIMITY_FACTOR values of the reference's published figure
(average_score_by_demonstration_proximity.png); the second form is simulator.py:169-200's
INITIAL_NOISE x NOISE_DECAY x 3 runs. Replica r of a configuration differs in its learner's seed
(seed + r): initial weights, replay sampling and target-smoothing noise.

--pbt-every N turns the grid into population-based training: after every N training steps the
members are scored on test episodes of --pbt-test-steps steps, the worst --pbt-frac of them take over
the learners and hyper-parameters of the best (PopulationTrainer.pbt_step) and perturb the fields
named by --pbt-explore within their bounds. One JSON line per exploit event, then the members'.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))

REFERENCE_STUDY = {"demo_factor": [10.0, 30.0, 50.0, 70.0]}


def parse_axis(text):
    """'name=v1,v2,...' -> (name, [values]); ints stay ints, everything else is a float."""
    name, _, values = text.partition("=")
    if not name or not values:
        raise argparse.ArgumentTypeError(f"--axis wants NAME=v1,v2,...: {text!r}")
    out = []
    for v in values.split(","):
        try:
            out.append(int(v))
        except ValueError:
            out.append(float(v))
    return name, out


def parse_explore(text):
    """'name=lo:hi' -> (name, (lo, hi))."""
    name, _, bounds = text.partition("=")
    lo, _, hi = bounds.partition(":")
    try:
        return name, (float(lo), float(hi))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--pbt-explore wants NAME=lo:hi: {text!r}")


def members_of(axes, replicas, seed):
    from nav.population import sweep_grid
    grid = sweep_grid(**axes)
    if replicas == 1:
        return [dict(m) for m in grid], [0] * len(grid)
    members, replica = [], []
    for m in grid:
        for r in range(replicas):
            members.append({**m, "seed": int(m.get("seed", seed)) + r})
            replica.append(r)
    return members, replica


def main(argv=None):
    from nav import config as K
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--axis", action="append", type=parse_axis, default=[],
                    metavar="NAME=v1,v2,...", help="one swept override; repeat for a grid")
    ap.add_argument("--reference-study", action="store_true",
                    help="demo_factor over 10, 30, 50, 70 (the reference's figure)")
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--envs-per-member", type=int, default=4096)
    ap.add_argument("--envs-per-group", type=int, default=1024)
    ap.add_argument("--train-steps", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="default: envs per member")
    ap.add_argument("--updates-per-step", type=int, default=2)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--learner", choices=("members", "batched"), default="members",
                    help="batched: every member's TD3 epoch in one launch per kernel "
                         "(needs --streams 1)")
    ap.add_argument("--test-steps", type=int, default=K.TEST_TIMEOUT * K.UPDATE_RATE)
    ap.add_argument("--seed", type=int, default=K.RANDOM_SEED)
    ap.add_argument("--no-demos", action="store_true")
    ap.add_argument("--pbt-every", type=int, default=0, metavar="N",
                    help="population-based training: an exploit / explore step after every N "
                         "training steps (0 = off)")
    ap.add_argument("--pbt-frac", type=float, default=0.25,
                    help="the share of the members replaced per step")
    ap.add_argument("--pbt-test-steps", type=int, default=200,
                    help="length of the test episodes the members are scored on")
    ap.add_argument("--pbt-explore", action="append", type=parse_explore, default=[],
                    metavar="NAME=lo:hi", help="a per-member field the clones perturb (x 0.8 or "
                                               "x 1.25, clipped to lo .. hi); repeatable")
    a = ap.parse_args(argv)
    axes = dict(a.axis)
    if a.reference_study:
        axes = {**REFERENCE_STUDY, **axes}
    if not axes:
        ap.error("nothing to sweep: give --axis NAME=v1,v2,... or --reference-study")
    if a.replicas < 1:
        ap.error("--replicas must be at least 1")
    members, replica = members_of(axes, a.replicas, a.seed)

    from nav.population import BC_KEYS, PBT_EXPLORE_KEYS, PopulationTrainer
    for name, _ in a.pbt_explore:
        if name not in PBT_EXPLORE_KEYS:
            ap.error(f"--pbt-explore {name}: cannot be explored; one of "
                     f"{sorted(PBT_EXPLORE_KEYS)}")
    tr = PopulationTrainer(members, envs_per_member=a.envs_per_member, hidden=a.hidden,
                           n_hidden=a.n_hidden, batch=a.batch or a.envs_per_member,
                           updates_per_step=a.updates_per_step, seed=a.seed,
                           envs_per_group=min(a.envs_per_group, a.envs_per_member),
                           demos=not a.no_demos, streams=a.streams, learner=a.learner)
    if a.pbt_every < 0:
        ap.error("--pbt-every must be at least 0")
    explore = dict(a.pbt_explore) or None
    for step in range(a.train_steps):
        tr.step()
        if a.pbt_every and (step + 1) % a.pbt_every == 0 and step + 1 < a.train_steps:
            seen = len(tr.pbt_history)
            tr.pbt_step(frac=a.pbt_frac, explore=explore, max_steps=a.pbt_test_steps)
            for ev in tr.pbt_history[seen:]:
                print(json.dumps({"pbt": ev}), flush=True)
    for m, row in enumerate(tr.evaluate(max_steps=a.test_steps)):
        if tr.bc:  # learning from the demonstrations: every member's three values, set or default
            row.update({k: tr.member_value(m, k) for k in BC_KEYS})
        if tr.env.demo_resets is not None:  # resets to demonstration states: value and share
            row.update(demo_reset_prob=tr.member_value(m, "demo_reset_prob"),
                       demo_reset_share=tr.demo_reset_share(m))
        print(json.dumps({"member": m, "replica": replica[m], "train_steps": a.train_steps,
                          **row}), flush=True)


if __name__ == "__main__":
    main()
