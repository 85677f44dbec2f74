"""Generate the committed golden fixtures by running the REFERENCE itself (container-only).

Imports /root/reference/environment.py and robot.py with two stub modules for dependencies that are
absent from the image: `pyglet` (graphics only; reached through robot.py:19 -> graphics.PathToDraw)
and `perlin_noise` (environment.py:7, used only by set_dynamics). The dynamics fields are injected
instead of generated, so every vector below is exercised through the reference's own code.

Writes small .npz files next to this script:
  dynamics.npz  Environment.dynamics/step on 4096 (state, action) cases incl. NaN/inf/clip/edges
  rng_init.npz  np.random.seed(s) -> set_init_and_goal + 3 resets, 32 seeds, + stream position
  trace.npz     headless robot-learning.py tick loop (3 CEM demos + 400 training ticks): the demo
                set, per-step (s, a, r, s', done), tick types, Robot counters and flags
  actions.npz   Robot.get_next_action_training/testing with generator-defined actor weights
  td3.npz       TD3.td3_update(4 epochs) with generator weights, injected batches and randn noise
  td3_grads.npz the same run's first param.grad of each optimizer (train_critic's two
                loss.backward(), robot.py:355-363; train_actor's, robot.py:393-395): the small
                tensors whole, the hidden x hidden weights as 4096 sampled entries + digests
  trace_branches.npz  trace.npz's loop and keys on a constant field (speed 1, angle 0.5) with the
                step ticks' actions SCRIPTED (BranchScript), so that the branches trace.npz never
                takes all occur; plus, per tick, step_goal / step_stuck (goal_reached / stuck_flag
                right after process_transition; -1 off the step ticks), step_blocked (env.step
                returned the unchanged state object), step_clipped (environment.py:117 clipped);
                and hand_*: one hand-made demonstration that ends inside the goal radius, as
                process_demonstration pushed it. Holds (tests/test_oracle_branches_cpu.py asserts
                it on the committed file): <= 800 step ticks; >= 8 with goal_reached; >= 6 done
                at >= 3 path lengths; >= 6 stuck; >= 1 each of goal & stuck, goal & done, done &
                stuck; >= 5 blocked (NaN actions: the only way past the clip) and >= 5 clipped at
                a world edge; >= 2 episodes whose FIRST step is stuck because the check still
                sees the previous episode's states; no goal distance within 1e-6 of 5, no
                stuck-check difference within 1e-6 of 2
  trace_branches_field.npz  the same scripted loop on make_fields(5), another numpy seed (kept
                in `seed`, as in trace_branches.npz): steering home through the field reaches the
                goal or sticks in a slow region, zigzags end by length, NaN actions block. Holds:
                <= 800 step ticks, >= 5 goal, >= 2 done, >= 3 stuck, >= 5 blocked steps, and the
                same two margins
  test_episodes.npz  the testing branch of update() (robot-learning.py:104-117) with a step cap
                instead of the wall clock; per step: state, action, next state, distance, the
                actor's residual, blocked / clipped; per episode: goal, start, the 1-based step
                at which distance <= 5 first held (-1: never) and test_best_distance as the
                reference leaves it. a_*: 24 episodes of <= 12 steps on make_fields(3) with the
                actor make_mlp_params(11, [2, 200, 200, 200, 2]) (>= 5 reached, >= 5 not, no
                distance within 1e-3 of 5, a pair count that is no multiple of 64, >= 3 steps
                clipped at an edge); b_*: 25 homing episodes on the constant field with an
                all-zero actor at a cap of 24 (all reach, in 1 to 17 steps; no distance within
                1e-6 of 5) and b6_*: the same under a cap of 6 (>= 5 reached, >= 5 cut off)

Usage: python tests/golden/make_golden.py [--only trace_branches,test_episodes]
(skips cleanly when /root/reference is absent; --only leaves the other files as they are)
"""
import argparse
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))


def import_reference():
    sys.path.insert(0, REF)
    sys.modules.setdefault("pyglet", types.ModuleType("pyglet"))
    pn = types.ModuleType("perlin_noise")

    class PerlinNoise:  # never called: fields are injected
        def __init__(self, octaves=1, seed=None):
            raise RuntimeError("perlin_noise is not available; inject dynamics fields")

    pn.PerlinNoise = PerlinNoise
    sys.modules["perlin_noise"] = pn
    import environment  # noqa: E402
    import robot  # noqa: E402
    return environment, robot


def make_fields(seed):
    """Synthetic fields with the value ranges set_dynamics produces (speed = sigmoid-stretched in
    (0,1), angle in [0,1]); float32 [100,100], x-major like environment.py:67-95."""
    rng = np.random.default_rng(seed)
    x = np.linspace(0, 1, 100)
    base = np.zeros((100, 100))
    for k in range(1, 6):
        ph = rng.uniform(0, 2 * np.pi, 2)
        base += rng.uniform(0.2, 1.0) * np.outer(np.sin(2 * np.pi * k * x + ph[0]),
                                                  np.cos(2 * np.pi * k * x + ph[1]))
    base += 0.3 * rng.standard_normal((100, 100))
    n = (base - base.min()) / (base.max() - base.min())
    speed = (1 / (1 + np.exp(-10 * (n - 0.5)))).astype(np.float32)
    ang = rng.standard_normal((100, 100)).cumsum(0).cumsum(1)
    angle = ((ang - ang.min()) / (ang.max() - ang.min())).astype(np.float32)
    return speed, angle


def new_env(environment, speed, angle):
    e = environment.Environment.__new__(environment.Environment)
    e.robot_state = np.array([0.0, 0.0], dtype=np.float32)
    e.robot_init_region = np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32)
    e.goal_state = np.array([0.0, 0.0], dtype=np.float32)
    e.dynamics_speed = speed
    e.dynamics_angle = angle
    return e


def gen_dynamics(environment):
    speed, angle = make_fields(1)
    env = new_env(environment, speed, angle)
    rng = np.random.default_rng(2)
    K = 4096
    s = rng.uniform(0, 100, (K, 2))
    a = rng.uniform(-7, 7, (K, 2))
    # edge cases: integer cell boundaries, world edges, the clip value, [99,100) reachable by reset
    s[:64] = np.floor(s[:64])
    s[64:128] = np.floor(s[64:128]) + 1 - 1e-9
    s[128:136] = [[0, 0], [98.9999, 98.9999], [0, 98.9999], [98.9999, 0], [99.5, 99.9], [99.99, 3],
                  [50, 50], [1e-300, 5]]
    a[136:144] = [[np.nan, 1], [1, np.nan], [np.inf, 0], [-np.inf, -np.inf], [0, 0], [5, 5],
                  [-5, 5], [1e9, -1e9]]
    a[144:208] = rng.uniform(-0.01, 0.01, (64, 2))  # tiny moves
    a[208:272] = rng.uniform(-300, 300, (64, 2))  # heavy clipping
    dyn = np.zeros((K, 2))
    stepped = np.zeros((K, 2))
    committed = np.zeros(K, np.int8)
    for i in range(K):
        dyn[i] = env.dynamics(s[i].copy(), a[i].copy())
        env.robot_state = s[i].copy()
        before = env.robot_state
        out = env.step(a[i].copy())
        stepped[i] = out
        committed[i] = 0 if out is before else 1
    np.savez_compressed(os.path.join(OUT, "dynamics.npz"), speed=speed, angle=angle, state=s,
                        action=a, dynamics=dyn, step=stepped, committed=committed)


def gen_rng_init(environment):
    seeds = np.array([1707366464, 0, 1, 2, 3, 42, 7, 99, 123, 1000, 2024, 31337] +
                     list(range(10, 30)), np.uint32)
    regions, goals, resets, tails = [], [], [], []
    speed, angle = make_fields(1)
    for sd in seeds:
        np.random.seed(int(sd))
        env = new_env(environment, speed, angle)
        env.set_init_and_goal()
        regions.append(np.asarray(env.robot_init_region, np.float64))
        goals.append(np.asarray(env.goal_state, np.float64))
        resets.append([env.reset().copy() for _ in range(3)])
        tails.append(np.random.random_sample(4))
    np.savez_compressed(os.path.join(OUT, "rng_init.npz"), seeds=seeds, region=np.array(regions),
                        goal=np.array(goals), resets=np.array(resets), tail=np.array(tails))


def gen_trace(environment, robot, n_ticks=400):
    """Headless copy of robot-learning.py:54-101 with the money budget removed; torch seeded only to
    make this generator reproducible; td3_update stubbed (it consumes no numpy draws, and the trace
    records the actions, so the learner does not influence what is checked)."""
    import torch
    torch.manual_seed(0)
    np.random.seed(1707366464)
    speed, angle = make_fields(3)
    env = new_env(environment, speed, angle)
    env.set_init_and_goal()
    state = env.reset()
    rb = robot.Robot(env.goal_state)
    rb.td3_agent.td3_update = lambda memory: None
    pushes = []
    orig_push = rb.memory.push

    def push(s, a, r, s2, d):
        pushes.append((np.array(s, np.float64), np.array(a, np.float64), float(r),
                       np.array(s2, np.float64), bool(d)))
        orig_push(s, a, r, s2, d)

    rb.memory.push = push
    types_, tick_state, tick_action, tick_next, push_idx = [], [], [], [], []
    ctr = []  # after each tick: plan_index, path_length, num_episodes, goal, stuck, demo, noise
    demos = []
    for _ in range(n_ticks):
        t = rb.get_next_action_type(state, 100.0)
        types_.append({"step": 0, "demo": 1, "reset": 2}[t])
        a = np.full(2, np.nan)
        ns = np.full(2, np.nan)
        s_in = np.array(state, np.float64)
        k_before = len(pushes)
        if t == "reset":
            state = env.reset()
            ns = np.array(state, np.float64)
        elif t == "demo":
            ds, da = env.get_demonstration()
            demos.append((ds.copy(), da.copy()))
            rb.process_demonstration(ds, da, 100.0)
        else:
            a = rb.get_next_action_training(state, 100.0)
            ns_ = env.step(a)
            rb.process_transition(state, a, ns_, 100.0)
            state = ns_
            ns = np.array(ns_, np.float64)
        tick_state.append(s_in)
        tick_action.append(np.array(a, np.float64))
        tick_next.append(ns)
        push_idx.append((k_before, len(pushes)))
        ctr.append((rb.plan_index, rb.path_length, rb.num_episodes, int(rb.goal_reached),
                    int(rb.stuck_flag), int(rb.demo_flag), rb.current_noise_scale))
    demo_set = np.array([np.asarray(x, np.float64) for x in rb.demonstration_states])
    P = pushes
    np.savez_compressed(
        os.path.join(OUT, "trace.npz"), speed=speed, angle=angle,
        goal=np.asarray(env.goal_state, np.float64),
        region=np.asarray(env.robot_init_region, np.float64), demo_set=demo_set,
        demo_states=np.array([d[0] for d in demos]), demo_actions=np.array([d[1] for d in demos]),
        tick_type=np.array(types_, np.int8), tick_state=np.array(tick_state),
        tick_action=np.array(tick_action), tick_next=np.array(tick_next),
        push_idx=np.array(push_idx, np.int32),
        push_s=np.array([p[0] for p in P]), push_a=np.array([p[1] for p in P]),
        push_r=np.array([p[2] for p in P]), push_s2=np.array([p[3] for p in P]),
        push_d=np.array([p[4] for p in P]), counters=np.array(ctr, np.float64))


WORLD_MAX = 100 - 1.0001  # the clip of environment.py:117


def constant_fields():
    """speed 1, angle 0.5: the rotation is pi, so action a moves the robot by -a (up to rounding)
    and every scripted episode below is predictable."""
    return np.full((100, 100), 1.0, np.float32), np.full((100, 100), 0.5, np.float32)


class BranchScript:
    """The actions of gen_trace_branches' step ticks: one scripted kind per training episode, each
    built to end the episode through a chosen branch of process_transition /
    get_next_action_type. Reads the Robot's counters and stuck history; changes nothing."""

    def __init__(self, env, rb, kinds):
        self.env, self.rb, self.kinds = env, rb, list(kinds)
        self.ep = -1
        self.mem = {}

    def begin_episode(self):
        self.ep += 1
        self.mem = {"t": 0}

    @property
    def kind(self):
        return self.kinds[self.ep]

    def exhausted(self):
        return self.ep + 1 >= len(self.kinds)

    def would_stick(self, state):
        prev = self.rb.previous_states
        return len(prev) >= 5 and all(np.linalg.norm(np.array(state) - np.array(q)) < 2
                                      for q in prev[-5:])

    @staticmethod
    def to(state, target):
        """the action that moves towards `target`, at most 5 per axis"""
        return -np.clip(np.asarray(target, np.float64) - state, -5.0, 5.0)

    def zigzag(self, m):
        m["zz"] = not m.get("zz", False)
        return np.array([5.0, 5.0]) if m["zz"] else np.array([-5.0, -5.0])

    def next_reset(self):
        """the state the next env.reset() will draw (no numpy draw happens before it)"""
        st = np.random.get_state()
        nxt = self.env.get_random_robot_init_state()
        np.random.set_state(st)
        return nxt

    def action(self, state):
        rb, m = self.rb, self.mem
        state = np.asarray(state, np.float64)
        goal = np.asarray(rb.goal_state, np.float64)
        m["t"] += 1
        t = m["t"]
        left = (rb.path_length - 1) - rb.plan_index  # steps after this one
        u = m.setdefault("u", (state - goal) / np.linalg.norm(state - goal))
        kind = self.kind
        if kind == "home":
            return np.clip(state - goal, -5.0, 5.0)
        if kind == "steer_home":  # any field: undo the cell's rotation and speed, head home
            cx, cy = int(state[0]), int(state[1])
            rot = -float(self.env.dynamics_angle[cx, cy]) * 2 * np.pi
            d = (goal - state) / max(float(self.env.dynamics_speed[cx, cy]), 1e-3)
            a = np.array([np.cos(rot) * d[0] - np.sin(rot) * d[1],
                          np.sin(rot) * d[0] + np.cos(rot) * d[1]])
            return a * min(1.0, 5.0 / np.abs(a).max())
        if kind in ("creep", "nan"):
            if kind == "nan":  # environment.py:125 is false for a NaN next state: a blocked step
                return np.array([np.nan, 1.0]) if t % 2 else np.array([np.nan, np.nan])
            return np.array([0.05 + 0.01 * t, -0.07])
        if kind == "goal_stuck":  # home to 5.4 from the goal, creep, step in as the check fires
            stage = goal + 5.4 * u
            if not m.get("staged"):
                if np.linalg.norm(stage - state) < 1e-9:
                    m["staged"] = True
                else:
                    return self.to(state, stage)
            if self.would_stick(state):
                return self.to(state, goal + 4.4 * u)
            w = np.array([-u[1], u[0]])
            return self.to(state, stage + 0.12 * (m["t"] % 3) * w + 0.05 * (m["t"] % 2) * u)
        if kind == "goal_done":  # wait 6.5 / 9 from the goal, step in at the path's last step
            q1, q2 = goal + 6.5 * u, goal + 9.0 * u
            if left == 0 and m.get("staged"):
                return self.to(state, goal + 4.2 * u)
            if not m.get("staged"):
                if np.linalg.norm(q1 - state) < 1e-9:
                    m["staged"] = True
                else:
                    return self.to(state, q1)
            m["at2"] = not m.get("at2", False)
            return self.to(state, q2 if m["at2"] else q1)
        if kind == "done_stuck":  # zigzag, then creep so that the check fires at the last step
            if left <= 5:
                return np.array([0.04 * (left + 1), 0.06])
            return self.zigzag(m)
        # the zigzag kinds: +-5 on both axes, ended by the path length
        if kind == "zig_edge":  # walk to the nearest world edge and push into it, sliding along
            if "edge" not in m:
                d = [state[0], WORLD_MAX - state[0], state[1], WORLD_MAX - state[1]]
                m["edge"] = int(np.argmin(d))
            e = m["edge"]
            ax, wall = e // 2, (0.0 if e % 2 == 0 else WORLD_MAX)
            if 2 <= t <= 15:
                tgt = state.copy()
                tgt[ax] = wall - 5.0 if wall == 0.0 else wall + 5.0  # past the edge
                tgt[1 - ax] = state[1 - ax] + (5.0 if t % 2 else -5.0)
                return -(np.clip(tgt - state, -5.0, 5.0))
            if t in (20, 23, 26):
                return np.array([np.nan, np.nan])
            if t in (29, 32):
                return np.array([2.0, np.nan])
        if kind == "zig_hover" and left <= 14:
            # hover +-1.2 around the next reset state: the next episode's first stuck check sees
            # five states of this one within 2 of its start
            p = m.setdefault("p", self.next_reset())
            off = np.array([1.2, 0.0]) if 1.3 < p[0] < WORLD_MAX - 1.3 else np.array([0.0, 1.2])
            a, b = p + off, p - off
            if not m.get("staged"):
                if np.linalg.norm(a - state) < 1e-9:
                    m["staged"] = True
                else:
                    return self.to(state, a)
            m["at2"] = not m.get("at2", False)
            return self.to(state, b if m["at2"] else a)
        return self.zigzag(m)


BRANCH_EPISODES = ("zig_edge", "goal_done", "done_stuck", "zig", "zig_hover", "creep", "zig_hover",
                   "creep", "home", "home", "goal_stuck", "creep", "home", "nan", "home", "home",
                   "creep", "home", "home")


def run_scripted_trace(environment, robot, speed, angle, seed, kinds):
    """gen_trace's headless tick loop with the step ticks' actions taken from a BranchScript
    instead of get_next_action_training (actions.npz pins that); ends after the reset tick that
    follows the last scripted episode. Returns the arrays of trace.npz plus, per tick, the step's
    goal_reached / stuck_flag right after process_transition, whether env.step returned the
    unchanged state object (blocked) and whether environment.py:117 clipped the step."""
    import torch
    torch.manual_seed(0)
    np.random.seed(seed)
    env = new_env(environment, speed, angle)
    env.set_init_and_goal()
    state = env.reset()
    rb = robot.Robot(env.goal_state)
    rb.td3_agent.td3_update = lambda memory: None
    pushes = []
    orig_push = rb.memory.push

    def push(s, a, r, s2, d):
        pushes.append((np.array(s, np.float64), np.array(a, np.float64), float(r),
                       np.array(s2, np.float64), bool(d)))
        orig_push(s, a, r, s2, d)

    rb.memory.push = push
    script = BranchScript(env, rb, kinds)
    types_, tick_state, tick_action, tick_next, push_idx, ctr, demos = [], [], [], [], [], [], []
    step_goal, step_stuck, blocked, clipped = [], [], [], []
    min_goal_margin = min_stuck_margin = np.inf
    while True:
        t = rb.get_next_action_type(state, 100.0)
        types_.append({"step": 0, "demo": 1, "reset": 2}[t])
        a = np.full(2, np.nan)
        ns = np.full(2, np.nan)
        s_in = np.array(state, np.float64)
        k_before = len(pushes)
        sg = ss = bl = cl = -1
        if t == "reset":
            state = env.reset()
            ns = np.array(state, np.float64)
            if script.exhausted():
                t = "end"
            else:
                script.begin_episode()
        elif t == "demo":
            ds, da = env.get_demonstration()
            demos.append((ds.copy(), da.copy()))
            rb.process_demonstration(ds, da, 100.0)
        else:
            a = script.action(state)
            hist = [np.array(q, np.float64) for q in rb.previous_states[-5:]]
            ns_ = env.step(a)
            bl = int(ns_ is state)
            rb.process_transition(state, a, ns_, 100.0)
            sg, ss = int(rb.goal_reached), int(rb.stuck_flag)
            ns = np.array(ns_, np.float64)
            cl = int(bool(np.any(ns == 0.0) or np.any(ns == WORLD_MAX)))
            # the margins of the two thresholds a last-bit difference could cross
            min_goal_margin = min(min_goal_margin,
                                  abs(np.linalg.norm(ns - np.asarray(env.goal_state)) - 5.0))
            if len(hist) >= 5:
                for q in hist:
                    min_stuck_margin = min(min_stuck_margin, abs(np.linalg.norm(s_in - q) - 2.0))
            state = ns_
        tick_state.append(s_in)
        tick_action.append(np.array(a, np.float64))
        tick_next.append(ns)
        push_idx.append((k_before, len(pushes)))
        ctr.append((rb.plan_index, rb.path_length, rb.num_episodes, int(rb.goal_reached),
                    int(rb.stuck_flag), int(rb.demo_flag), rb.current_noise_scale))
        step_goal.append(sg)
        step_stuck.append(ss)
        blocked.append(bl)
        clipped.append(cl)
        if t == "end":
            break
    assert min_goal_margin > 1e-6 and min_stuck_margin > 1e-6, (min_goal_margin, min_stuck_margin)
    P = pushes
    return dict(
        seed=seed, speed=speed, angle=angle, goal=np.asarray(env.goal_state, np.float64),
        region=np.asarray(env.robot_init_region, np.float64),
        demo_set=np.array([np.asarray(x, np.float64) for x in rb.demonstration_states]),
        demo_states=np.array([d[0] for d in demos]), demo_actions=np.array([d[1] for d in demos]),
        tick_type=np.array(types_, np.int8), tick_state=np.array(tick_state),
        tick_action=np.array(tick_action), tick_next=np.array(tick_next),
        push_idx=np.array(push_idx, np.int32),
        push_s=np.array([p[0] for p in P]), push_a=np.array([p[1] for p in P]),
        push_r=np.array([p[2] for p in P]), push_s2=np.array([p[3] for p in P]),
        push_d=np.array([p[4] for p in P]), counters=np.array(ctr, np.float64),
        step_goal=np.array(step_goal, np.int8), step_stuck=np.array(step_stuck, np.int8),
        step_blocked=np.array(blocked, np.int8), step_clipped=np.array(clipped, np.int8))


def gen_hand_demo(robot, goal):
    """One hand-made demonstration that ends inside the goal radius, pushed by the reference's
    own process_demonstration (a fresh Robot: demonstration_states empty before it, demo_flag
    false, as at the reference's first demo tick). float32 paths, as get_demonstration returns."""
    T = 24
    k = np.arange(T, dtype=np.float64)[:, None]
    start = goal + np.array([31.0, 22.5]) * np.where(np.asarray(goal) > 50.0, -1.0, 1.0)
    st = start + (goal + np.array([0.8, -0.6]) - start) * (k / (T - 1)) ** 0.8
    st += 0.37 * np.stack([np.sin(1.7 * k[:, 0]), np.cos(2.3 * k[:, 0])], 1)
    st = st.astype(np.float32)
    ac = np.clip(st[:-1] - st[1:], -7.0, 7.0)  # raw actions may pass the +-5 clamp
    ac = np.concatenate([ac, [[0.3, -0.2]]]).astype(np.float32)
    rb = robot.Robot(np.asarray(goal, np.float64))
    pushes = []
    rb.memory.push = lambda s, a, r, s2, d: pushes.append(
        (np.array(s, np.float64), np.array(a, np.float64), float(r), np.array(s2, np.float64),
         bool(d)))
    state = np.random.get_state()
    np.random.seed(7)  # the augmentation's draws
    rb.process_demonstration(st, ac, 100.0)
    np.random.set_state(state)
    assert len(pushes) == T - 1
    return dict(hand_states=st, hand_actions=ac,
                hand_push_s=np.array([p[0] for p in pushes]),
                hand_push_a=np.array([p[1] for p in pushes]),
                hand_push_r=np.array([p[2] for p in pushes]),
                hand_push_s2=np.array([p[3] for p in pushes]),
                hand_push_d=np.array([p[4] for p in pushes]))


def gen_trace_branches(environment, robot):
    speed, angle = constant_fields()
    out = run_scripted_trace(environment, robot, speed, angle, 1707366464, BRANCH_EPISODES)
    out.update(gen_hand_demo(robot, out["goal"]))
    np.savez_compressed(os.path.join(OUT, "trace_branches.npz"), **out)
    print("trace_branches:", branch_counts(out))


FIELD_EPISODES = ("zig", "steer_home", "steer_home", "creep", "steer_home", "zig", "steer_home",
                  "steer_home", "nan", "steer_home", "steer_home")


def gen_trace_branches_field(environment, robot):
    """The same loop on a make_fields field, for variety in the dynamics and the demonstration
    term: steering home through the field reaches the goal or sticks in a slow region."""
    speed, angle = make_fields(5)
    out = run_scripted_trace(environment, robot, speed, angle, 20240229, FIELD_EPISODES)
    np.savez_compressed(os.path.join(OUT, "trace_branches_field.npz"), **out)
    print("trace_branches_field:", branch_counts(out))


def branch_counts(t):
    """The counts tests/test_oracle_branches_cpu.py asserts on the committed file."""
    step = t["tick_type"] == 0
    lo = t["push_idx"][step, 0]
    d = t["push_d"][lo].astype(bool)
    g, s = t["step_goal"][step] == 1, t["step_stuck"][step] == 1
    return dict(step=int(step.sum()), demo=int((t["tick_type"] == 1).sum()),
                reset=int((t["tick_type"] == 2).sum()), goal=int(g.sum()), done=int(d.sum()),
                stuck=int(s.sum()), goal_stuck=int((g & s).sum()), goal_done=int((g & d).sum()),
                done_stuck=int((d & s).sum()), blocked=int((t["step_blocked"][step] == 1).sum()),
                clipped=int((t["step_clipped"][step] == 1).sum()),
                done_path_lengths=sorted(set(t["counters"][step, 1][d].astype(int).tolist())))


def load_net(net, params):
    import torch
    layers = [m for m in net.modules() if isinstance(m, torch.nn.Linear)]
    assert len(layers) == len(params)
    with torch.no_grad():
        for lin, (W, b) in zip(layers, params):
            lin.weight.copy_(torch.tensor(W))
            lin.bias.copy_(torch.tensor(b))


def gen_actions(environment, robot):
    sys.path.insert(0, ROOT)
    from oracle.td3_oracle import make_mlp_params
    import torch
    torch.manual_seed(0)
    actor_p = make_mlp_params(11, [2, 200, 200, 200, 2])
    rb = robot.Robot(np.array([60.0, 40.0]))
    load_net(rb.td3_agent.actor_network, actor_p)
    rng = np.random.default_rng(5)
    K = 64
    states = rng.uniform(0, 100, (K, 2))
    goals = rng.uniform(5, 95, (K, 2))
    sigmas = 0.75 ** rng.integers(0, 12, K)
    seeds = rng.integers(0, 2**31, K)
    a_tr, a_te, res, z = [], [], [], []
    for i in range(K):
        rb.goal_state = goals[i]
        rb.current_noise_scale = float(sigmas[i])
        np.random.seed(int(seeds[i]))
        a_tr.append(rb.get_next_action_training(states[i].copy(), 0.0))
        np.random.seed(int(seeds[i]))
        z.append(np.random.normal(0, 1, 2))
        a_te.append(rb.get_next_action_testing(states[i].copy()))
        res.append(rb.residual_action(states[i] - goals[i]))
    np.savez_compressed(os.path.join(OUT, "actions.npz"), actor_seed=11, states=states, goals=goals,
                        sigmas=sigmas, action_train=np.array(a_tr), action_test=np.array(a_te),
                        residual=np.array(res, np.float32), z=np.array(z))


def run_test_episode(environment, env, rb, start, goal, cap):
    """The testing branch of update() (robot-learning.py:104-117), headless, the wall-clock
    timeout replaced by a cap of `cap` steps. Returns the per-step records, the step at which
    distance <= TEST_DISTANCE_THRESHOLD first held (1-based; -1: never) and test_best_distance as
    the reference leaves it: updated with `<` AFTER the threshold test, so never by the reaching
    step itself (the reference reports it only for an episode that did not reach the goal)."""
    import constants
    env.robot_state = np.array(start, np.float64)
    env.goal_state = np.array(goal, np.float64)
    rb.goal_state = env.goal_state
    state = env.robot_state
    best = np.inf
    reached = -1
    rec = []
    for t in range(cap):
        res = rb.residual_action(state - rb.goal_state)
        action = rb.get_next_action_testing(state)
        next_state = env.step(action)
        distance = np.linalg.norm(next_state - env.goal_state)
        rec.append((np.array(state, np.float64), np.array(action, np.float64),
                    np.array(next_state, np.float64), float(distance),
                    np.array(res, np.float32), int(next_state is state),
                    int(bool(np.any(next_state == 0.0) or np.any(next_state == WORLD_MAX)))))
        state = next_state
        if distance <= constants.TEST_DISTANCE_THRESHOLD:
            reached = t + 1
            break
        if distance < best:
            best = distance
    return rec, reached, best


def pack_episodes(prefix, episodes, goals, starts):
    """flat per-(episode, step) arrays + per-episode arrays"""
    flat = [(e, t) + r for e, (rec, _, _) in enumerate(episodes) for t, r in enumerate(rec)]
    col = lambda k, dt: np.array([f[k] for f in flat], dt)  # noqa: E731
    return {prefix + "ep": col(0, np.int32), prefix + "t": col(1, np.int32),
            prefix + "state": col(2, np.float64), prefix + "action": col(3, np.float64),
            prefix + "next": col(4, np.float64), prefix + "dist": col(5, np.float64),
            prefix + "residual": col(6, np.float32), prefix + "blocked": col(7, np.int8),
            prefix + "clipped": col(8, np.int8),
            prefix + "goal": np.array(goals, np.float64),
            prefix + "start": np.array(starts, np.float64),
            prefix + "reached_step": np.array([e[1] for e in episodes], np.int32),
            prefix + "best": np.array([e[2] for e in episodes], np.float64)}


def gen_test_episodes(environment, robot):
    sys.path.insert(0, ROOT)
    from oracle.td3_oracle import make_mlp_params
    import torch
    torch.manual_seed(0)
    out = {}
    # group (a): a make_fields field, a generator-defined actor, 24 episodes of at most 12 steps;
    # a third start 5 to 7 from the goal, a third hard on a world edge, the rest anywhere
    actor_seed, cap_a = 11, 12
    speed, angle = make_fields(3)
    env = new_env(environment, speed, angle)
    rb = robot.Robot(np.array([50.0, 50.0]))
    load_net(rb.td3_agent.actor_network, make_mlp_params(actor_seed, [2, 200, 200, 200, 2]))
    rng = np.random.default_rng(17)
    goals = rng.uniform(8, 92, (24, 2))
    starts = rng.uniform(1, 98, (24, 2))
    # the field turns most actions away from the goal, so the near starts are drawn until the
    # reference reaches the goal from eight of them, four of those in more than one step
    k = late = 0
    while k < 8:
        gl, th = rng.uniform(8, 92, 2), rng.uniform(0, 2 * np.pi)
        st = gl + rng.uniform(5.2, 7.0) * np.array([np.cos(th), np.sin(th)])
        _, reached, _ = run_test_episode(environment, env, rb, st, gl, cap_a)
        if reached < 1 or (reached == 1 and k - late >= 4):
            continue
        goals[k], starts[k] = gl, st
        late += reached > 1
        k += 1
    for k in range(8, 16):  # on or next to an edge
        starts[k, k % 2] = (0.02, 98.97, 0.0, WORLD_MAX)[(k // 2) % 4]
    eps = [run_test_episode(environment, env, rb, starts[k], goals[k], cap_a) for k in range(24)]
    assert sum(e[1] > 0 for e in eps) >= 8 and len([1 for e in eps for _ in e[0]]) % 64
    out.update(pack_episodes("a_", eps, goals, starts), a_speed=speed, a_angle=angle,
               a_actor_seed=actor_seed, a_cap=cap_a)
    assert np.abs(out["a_dist"] - 5.0).min() > 1e-3
    # group (b): the constant field, an all-zero actor (the residual is exactly 0), one goal,
    # starts on a spiral; every episode at a cap past the longest one and at a cap of 6
    speed, angle = constant_fields()
    env = new_env(environment, speed, angle)
    rb = robot.Robot(np.array([8.0, 9.0]))
    with torch.no_grad():
        for prm in rb.td3_agent.actor_network.parameters():
            prm.zero_()
    g = np.array([8.0, 9.0])
    i = np.arange(0, 97, 4)
    r, th = 5.5 + 0.85 * i, 0.1 + 1.3 * i / 96
    starts = g + r[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    goals = np.broadcast_to(g, starts.shape).copy()
    cap_b = 24
    eps = [run_test_episode(environment, env, rb, s, g, cap_b) for s in starts]
    eps6 = [run_test_episode(environment, env, rb, s, g, 6) for s in starts]
    out.update(pack_episodes("b_", eps, goals, starts), b_cap=cap_b,
               b6_reached_step=np.array([e[1] for e in eps6], np.int32),
               b6_best=np.array([e[2] for e in eps6], np.float64),
               b6_final=np.array([e[0][-1][2] for e in eps6], np.float64),
               b6_steps=np.array([len(e[0]) for e in eps6], np.int32))
    assert np.abs(out["b_dist"] - 5.0).min() > 1e-6
    assert np.all(out["b_residual"] == 0)
    np.savez_compressed(os.path.join(OUT, "test_episodes.npz"), **out)
    for p in ("a_", "b_"):
        rs = out[p + "reached_step"]
        print("test_episodes", p, "pairs", len(out[p + "ep"]), "reached", int((rs > 0).sum()),
              "unreached", int((rs < 0).sum()), "steps", sorted(set(rs.tolist())),
              "blocked", int(out[p + "blocked"].sum()), "clipped", int(out[p + "clipped"].sum()))
    print("test_episodes b6 reached", int((out["b6_reached_step"] > 0).sum()))


def gen_td3(robot, epochs=4, B=100, n_trans=300):
    sys.path.insert(0, ROOT)
    from oracle.td3_oracle import make_mlp_params, param_digest
    import torch
    torch.manual_seed(0)
    pa = make_mlp_params(21, [2, 200, 200, 200, 2])
    p1 = make_mlp_params(22, [4, 200, 200, 200, 1])
    p2 = make_mlp_params(23, [4, 200, 200, 200, 1])
    actor, c1, c2 = robot.Residual_Actor_Network(), robot.Residual_Critic_Network(), \
        robot.Residual_Critic_Network()
    load_net(actor, pa)
    load_net(c1, p1)
    load_net(c2, p2)
    agent = robot.TD3(actor, c1, c2)
    rng = np.random.default_rng(31)
    S = rng.uniform(0, 100, (n_trans, 2))
    A = rng.uniform(-5, 5, (n_trans, 2))
    R = rng.uniform(-500, 50, n_trans)
    S2 = np.clip(S + rng.uniform(-4, 4, (n_trans, 2)), 0, 98.9999)
    D = rng.random(n_trans) < 0.1
    n_samples = epochs + (epochs + 1) // 2
    idx = np.stack([rng.permutation(n_trans)[:B] for _ in range(n_samples)]).astype(np.int32)
    noise = rng.standard_normal((epochs, B, 2)).astype(np.float32)
    it = {"s": 0, "n": 0}

    class Buf:
        def sample(self, bs):
            i = idx[it["s"]]
            it["s"] += 1
            return S[i], A[i], R[i], S2[i], D[i]

    orig = torch.randn_like

    def fake_randn_like(x):
        t = torch.tensor(noise[it["n"]])
        it["n"] += 1
        return t

    closs, aloss = [], []
    agent_train_critic, agent_train_actor = agent.train_critic, agent.train_actor
    # the gradients the reference forms in loss.backward(), read at each optimizer's first step
    first_grads = {}

    def record(name, opt):
        step = opt.step

        def wrapped(*a, **k):
            if name not in first_grads:
                first_grads[name] = [p.grad.detach().clone() for g in opt.param_groups
                                     for p in g["params"]]
            return step(*a, **k)
        opt.step = wrapped

    record("critic1", agent.critic_optimizer_1)
    record("critic2", agent.critic_optimizer_2)
    record("actor", agent.actor_optimizer)

    def tc(rb):
        r = agent_train_critic(rb)
        closs.append(r)
        return r

    def ta(rb):
        r = agent_train_actor(rb)
        aloss.append(r)
        return r

    agent.train_critic, agent.train_actor = tc, ta
    agent.num_epochs = epochs
    torch.randn_like = fake_randn_like
    try:
        agent.td3_update(Buf())
    finally:
        torch.randn_like = orig
    nets = {"actor": agent.actor_network, "critic1": agent.critic_network_1,
            "critic2": agent.critic_network_2, "target_actor": agent.target_actor,
            "target_critic1": agent.target_critic_network_1,
            "target_critic2": agent.target_critic_network_2}
    out = dict(epochs=epochs, B=B, S=S, A=A, R=R, S2=S2, D=D, idx=idx, noise=noise,
               critic_loss=np.array(closs), actor_loss=np.array(aloss))
    for name, net in nets.items():
        dig = param_digest(list(net.parameters()))
        out[name + "_sum"] = np.array([d[0] for d in dig])
        out[name + "_sq"] = np.array([d[1] for d in dig])
        out[name + "_idx"] = np.array([d[2] for d in dig])
        out[name + "_val"] = np.array([d[3] for d in dig])
    probe = rng.uniform(0, 100, (16, 2)).astype(np.float32)
    probe_a = rng.uniform(-5, 5, (16, 2)).astype(np.float32)
    with torch.no_grad():
        out["probe_s"] = probe
        out["probe_a"] = probe_a
        out["probe_actor"] = agent.actor_network(torch.tensor(probe)).numpy()
        out["probe_q1"] = agent.critic_network_1(torch.tensor(probe), torch.tensor(probe_a)).numpy()
    np.savez_compressed(os.path.join(OUT, "td3.npz"), **out)
    gout = dict(critic_idx=idx[0], actor_idx=idx[1], noise=noise[0])
    grng = np.random.default_rng(99)
    for name, grads in first_grads.items():
        for t, g in enumerate(grads):
            a = g.numpy().astype(np.float32)
            key = f"{name}_{t}"
            if a.size <= 1024:
                gout[key] = a
            else:  # a hidden x hidden weight: sampled entries + whole-tensor digests
                ix = grng.integers(0, a.size, 4096)
                proj = np.random.default_rng(1000 + t).standard_normal(a.size)
                gout[key + "_idx"] = ix
                gout[key + "_val"] = a.ravel()[ix]
                gout[key + "_shape"] = np.array(a.shape)
                gout[key + "_dig"] = np.array([a.astype(np.float64).sum(),
                                               (a.astype(np.float64) ** 2).sum(),
                                               (a.astype(np.float64).ravel() * proj).sum()])
    np.savez_compressed(os.path.join(OUT, "td3_grads.npz"), **gout)


def main():
    if not os.path.isdir(REF):
        print("reference absent; fixtures are committed, nothing to do")
        return
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="comma-separated fixtures to write (file names "
                    "without .npz; td3 also writes td3_grads); default: all of them")
    only = [x for x in ap.parse_args().only.split(",") if x]
    environment, robot = import_reference()
    gens = {"dynamics": lambda: gen_dynamics(environment),
            "rng_init": lambda: gen_rng_init(environment),
            "actions": lambda: gen_actions(environment, robot),
            "td3": lambda: gen_td3(robot),
            "trace": lambda: gen_trace(environment, robot),
            "trace_branches": lambda: gen_trace_branches(environment, robot),
            "trace_branches_field": lambda: gen_trace_branches_field(environment, robot),
            "test_episodes": lambda: gen_test_episodes(environment, robot)}
    unknown = [x for x in only if x not in gens]
    if unknown:
        ap.error(f"unknown fixture(s) {unknown}; known: {sorted(gens)}")
    for name, fn in gens.items():
        if not only or name in only:
            fn()
    for f in sorted(os.listdir(OUT)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
