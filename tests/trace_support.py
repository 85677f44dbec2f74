"""Readers of the reference's trace fixtures (tests/golden/trace*.npz, test_episodes.npz) that the
CPU tests of the oracle and the GPU tests of the kernels share: both are held to the same files by
the same expectations."""
import numpy as np

from conftest import golden

BRANCH_TRACES = ("trace_branches.npz", "trace_branches_field.npz")  # scripted step actions
TRACES = ("trace.npz",) + BRANCH_TRACES
DEMO_CASES = ["trace", "trace_branches", "trace_branches_field", "hand"]
WORLD_MAX = 100 - 1.0001


def branch_counts(t):
    """Branch counts of a trace fixture that records step_goal / step_stuck (trace_branches.npz);
    for trace.npz the goal and stuck columns come from its counters."""
    step = t["tick_type"] == 0
    lo = t["push_idx"][step, 0]
    d = t["push_d"][lo].astype(bool)
    if "step_goal" in t.files:
        g, s = t["step_goal"][step] == 1, t["step_stuck"][step] == 1
        blocked = int((t["step_blocked"][step] == 1).sum())
        clipped = int((t["step_clipped"][step] == 1).sum())
    else:
        g, s = t["counters"][step, 3] == 1, t["counters"][step, 4] == 1
        ns = t["tick_next"][step]
        blocked = int(np.all(ns == t["tick_state"][step], axis=1).sum())
        clipped = int(((ns == 0.0) | (ns == WORLD_MAX)).any(1).sum())
    return dict(step=int(step.sum()), demo=int((t["tick_type"] == 1).sum()),
                reset=int((t["tick_type"] == 2).sum()), goal=int(g.sum()), done=int(d.sum()),
                stuck=int(s.sum()), goal_stuck=int((g & s).sum()), goal_done=int((g & d).sum()),
                done_stuck=int((d & s).sum()), blocked=blocked, clipped=clipped,
                done_path_lengths=sorted(set(t["counters"][step, 1][d].astype(int).tolist())))


def step_ticks(t):
    """(tick i, push row, reset state or None) of every step tick from the first one on."""
    types = t["tick_type"]
    first = int(np.nonzero(types == 0)[0][0])
    out = []
    for i in range(first, len(types)):
        if types[i] != 0:
            continue
        lo, hi = t["push_idx"][i]
        assert hi - lo == 1
        nxt = t["tick_next"][i + 1] if i + 1 < len(types) and types[i + 1] == 2 else None
        out.append((i, int(lo), nxt))
    return first, out


def want_flags(t, i, lo, reset_state):
    """The tick's flag bits 1 | 2 | 4 | 8 as the reference's records imply them: done = push_d,
    goal and stuck as they stood right after process_transition, ended = the reference's next
    tick is a reset."""
    return (int(bool(t["push_d"][lo])) | 2 * int(t["step_goal"][i] == 1) |
            4 * int(t["step_stuck"][i] == 1) | 8 * int(reset_state is not None))


def check_goal_row(t, i, lo, row_reward):
    """A goal row's reward is exactly GOAL_REWARD, or GOAL_REWARD - STUCK_PENALTY = 0 when the
    stuck check fired on the same step (robot.py:664-669)."""
    if t["step_goal"][i] == 1:
        want = 0.0 if t["step_stuck"][i] == 1 else 50.0
        assert t["push_r"][lo] == want and float(row_reward) == want, i


def init_mirror(orc, t, first):
    st = orc.VecAgentState(1)
    c = t["counters"]
    st.state[0] = t["tick_state"][first]
    st.goal[0] = t["goal"]
    st.region[0] = t["region"]
    st.plan_index[0] = int(c[first][0])
    st.path_length[0] = int(c[first][1])
    st.episodes[0] = int(c[first][2])
    st.noise_scale[0] = c[first][6]
    st.meta[0] = 4  # demo_flag
    return st


def carried_first_stuck(t):
    """Episodes whose FIRST step is stuck: only possible when the check still sees the previous
    episode's states (robot.py:425: previous_states is not cleared by Robot.reset)."""
    types = t["tick_type"]
    return [i for i in range(1, len(types))
            if types[i] == 0 and types[i - 1] == 2 and t["step_stuck"][i] == 1]


def demo_push_rows(t):
    """The reference's demonstration pushes of a trace fixture as replay rows in float32, in
    nav_demo_transitions' order (demonstration, step), and their float64 rewards."""
    rows, rew = [], []
    for i in np.nonzero(t["tick_type"] == 1)[0]:
        lo, hi = t["push_idx"][i]
        for k in range(lo, hi):
            rows.append(np.concatenate([t["push_s"][k], t["push_a"][k], [t["push_r"][k]],
                                        t["push_s2"][k], [float(t["push_d"][k])]]))
            rew.append(t["push_r"][k])
    return np.array(rows).astype(np.float32), np.array(rew, np.float64)


def hand_push_rows(t):
    rows = np.concatenate([t["hand_push_s"], t["hand_push_a"], t["hand_push_r"][:, None],
                           t["hand_push_s2"], t["hand_push_d"][:, None].astype(np.float64)], 1)
    return rows.astype(np.float32), t["hand_push_r"].astype(np.float64)


def assert_demo_rows(got, want, reward64):
    """State, action, next-state and done columns equal; the reward equal or within one float32
    ulp of float32(push_r) (the kernel's norm2 is sqrt(fma(y, y, x * x)), the reference's is
    np.linalg.norm); rows inside the goal radius exactly GOAL_REWARD. Returns the count of goal
    rows and of rewards that differ by an ulp."""
    assert got.shape == want.shape
    cols = [0, 1, 2, 3, 5, 6, 7]
    assert np.array_equal(got[:, cols], want[:, cols])
    r32 = reward64.astype(np.float32)
    ulp = np.abs(got[:, 4].view(np.int32).astype(np.int64) - r32.view(np.int32))
    assert ulp.max() <= 1, int(ulp.argmax())
    inside = reward64 == 50.0
    assert np.all(got[inside, 4] == 50.0) and not np.any(got[~inside, 4] == 50.0)
    return int(inside.sum()), int((ulp == 1).sum())


def demo_cases():
    """(name, states [n][T][2] f32, actions, goals [n][2], reference rows f32, rewards f64)."""
    out = []
    for name in TRACES:
        t = golden(name)
        n = len(t["demo_states"])
        rows, rew = demo_push_rows(t)
        out.append((name, t["demo_states"], t["demo_actions"], np.tile(t["goal"], (n, 1)), rows,
                    rew))
    t = golden("trace_branches.npz")
    rows, rew = hand_push_rows(t)
    out.append(("hand", t["hand_states"][None], t["hand_actions"][None], t["goal"][None], rows,
                rew))
    return out


def episode_slices(g, p):
    """per episode of group `p` ("a_" / "b_") of test_episodes.npz: the slice of its flat rows"""
    ep = g[p + "ep"]
    n = len(g[p + "goal"])
    idx = [np.nonzero(ep == e)[0] for e in range(n)]
    for e, ix in enumerate(idx):
        assert len(ix) and np.array_equal(g[p + "t"][ix], np.arange(len(ix))), e
    return idx
