"""Resets to demonstration states restated on the host (include/navenv.h, nav_demo_reset, and the
`usable` table of nav.demos.demo_reset_usable): oracle.philox for the draws, Python ints and
floats for u01 and the mul-hi index (pinned by hand-worked values in tests/test_demo_reset_cpu.py).
Needs no GPU and no libnavenv.so."""
import numpy as np

from oracle import oracle as O

NAV_TAG_DRESET = 9


def u01(hi, lo):
    """The 53-bit uniform in [0, 1) of two Philox words (numpy's random_sample formula)."""
    return ((hi >> 5) * 67108864.0 + (lo >> 6)) / 9007199254740992.0


def mulhi(w, n):
    """(w * n) >> 32: an index in [0, n) from one 32-bit word."""
    return (int(w) * int(n)) >> 32


def usable(states, goals, goal_threshold):
    """usable[j]: the leading states of demonstration j further than goal_threshold from its
    goal, clamped to 1 .. T - 1, by a plain loop."""
    states = np.asarray(states, np.float64)
    goals = np.asarray(goals, np.float64)
    J, T = states.shape[:2]
    out = np.empty(J, np.int32)
    for j in range(J):
        k = 0
        while k < T and float(np.hypot(*(states[j, k] - goals[j]))) > goal_threshold:
            k += 1
        out[j] = min(max(k, 1), T - 1)
    return out


def draw(e, ep, seed):
    """The four Philox words of env e's reset into episode ep."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(x) for x in O.philox((0, e & 0xFFFFFFFF, NAV_TAG_DRESET, ep & 0xFFFFFFFF), key)]


def reset(state, flags, episodes, seed, demo_states, usable_, n_demos, envs_per_group, prob,
          prob_group=None):
    """nav_demo_reset on the host. state [n][2] f64, flags [n] u8, episodes [n] i32, demo_states
    [G * n_demos][T][2] f32, usable_ [G * n_demos]. -> (the new state, counts [ceil(n/64)] int64
    of this launch alone, picks [n][2] int64: (demonstration d, time index t) of the envs that
    took a state, (-1, -1) elsewhere)."""
    state = np.array(state, np.float64, copy=True)
    demo = np.asarray(demo_states, np.float32)
    n = state.shape[0]
    counts = np.zeros((n + 63) // 64, np.int64)
    picks = np.full((n, 2), -1, np.int64)
    for e in range(n):
        if not int(flags[e]) & 8:
            continue
        g = e // envs_per_group
        w = draw(e, int(episodes[e]), seed)
        p = float(prob_group[g]) if prob_group is not None else float(prob)
        if u01(w[0], w[1]) < p:
            d = mulhi(w[2], n_demos)
            t = mulhi(w[3], int(usable_[g * n_demos + d]))
            state[e] = demo[g * n_demos + d, t].astype(np.float64)
            counts[e // 64] += 1
            picks[e] = (d, t)
    return state, counts, picks
