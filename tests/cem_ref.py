"""The CEM demonstrator (environment.py:140-179) and the demonstration augmentation
(robot.py:771-824) restated in plain numpy from their definitions: what k_rollout, k_cem_rollout,
k_cem_elite and k_demo_augment (csrc/demonstrator.hip) are held to. Imports no torch and not
nav._lib; the one library call is the oracle's norm2 (sqrt(fma(a1, a1, a0 * a0)), the kernels'
formula: numpy has no fma).

  dynamics(speed, angle, s, a)     Environment.dynamics on n (state, action) pairs, f64
  rollout(...)                     open-loop paths from given starts, f64, and their rewards
  cem_rollout(...)                 one CEM iteration's actions (f32), paths (f64 and f32), rewards
  elite(reward, actions, E)        order, float32 mean / std over the E best, best
  demonstrations(...)              the I-iteration loop over n problems, every iteration kept
  augment_points(...)              one demonstration's block of the augmented demonstration set
  tie_patterns / assert_decisive_gaps   the planted ties and the reward-gap precondition the
                                   CPU and GPU tests share

Tied rewards: the order is ascending reward, then path index (a stable sort). numpy's default
argsort does not promise an order for exact ties, so this rule is the project's definition there;
k_cem_elite implements the same rule.
"""
import numpy as np

from oracle import oracle as orc

WORLD = 100
MAX_ACTION = 5.0
HI = 100.0 - 1.0001     # the clip of environment.py:117
_TWO = np.float32(2.0)
_PI = np.float32(np.pi)


def dynamics(speed, angle, s, a):
    """environment.py:98-119 for s [n][2], a [n][2] (f64): actions clipped to +-5, the cell by
    truncation clamped to 0..99, rot = (angle * 2f) * pi_f a float32 product chain (NEP 50), the
    displacement speed * R(rot) a in f64 (the reference's speed * |a| * (cos, sin)(atan2 + rot) up
    to a few ulp), the result clipped to [0, 100 - 1.0001]."""
    s = np.asarray(s, np.float64).reshape(-1, 2)
    a = np.clip(np.asarray(a, np.float64).reshape(-1, 2), -MAX_ACTION, MAX_ACTION)
    cx = np.clip(s[:, 0].astype(np.int64), 0, WORLD - 1)
    cy = np.clip(s[:, 1].astype(np.int64), 0, WORLD - 1)
    rot = (np.asarray(angle, np.float32)[cx, cy] * _TWO) * _PI
    assert rot.dtype == np.float32
    rot = rot.astype(np.float64)
    sp = np.asarray(speed, np.float32)[cx, cy].astype(np.float64)
    cr, sr = np.cos(rot), np.sin(rot)
    out = np.empty_like(s)
    out[:, 0] = np.clip(s[:, 0] + sp * (a[:, 0] * cr - a[:, 1] * sr), 0.0, HI)
    out[:, 1] = np.clip(s[:, 1] + sp * (a[:, 0] * sr + a[:, 1] * cr), 0.0, HI)
    return out


def path_reward(final, goal):
    """environment.py:164, 182-183 on the float32 planning_paths row: -norm2(f64(f32(s_T)) - goal)
    for final [n][2] against goal [2] or [n][2]."""
    f = np.asarray(final).astype(np.float32).astype(np.float64).reshape(-1, 2)
    g = np.broadcast_to(np.asarray(goal, np.float64), f.shape)
    return np.array([-orc.norm2(f[i, 0] - g[i, 0], f[i, 1] - g[i, 1]) for i in range(len(f))])


def rollout(speed, angle, start, actions, goal=None):
    """Open-loop rollouts: start [P][2], actions [P][T][2] -> paths [P][T+1][2] f64 and, given a
    goal [2], the path rewards [P] (else None)."""
    start = np.asarray(start, np.float64).reshape(-1, 2)
    P = len(start)
    actions = np.asarray(actions, np.float64).reshape(P, -1, 2)
    T = actions.shape[1]
    paths = np.empty((P, T + 1, 2))
    paths[:, 0] = start
    for t in range(T):
        paths[:, t + 1] = dynamics(speed, angle, paths[:, t], actions[:, t])
    return paths, (None if goal is None else path_reward(paths[:, T], goal))


def region_sample(region, u):
    """environment.py:135-137: uniform([l, b], [r, t]) = low + (high - low) * u; region [n][4] =
    (left, right, bottom, top), u [n][2]."""
    region = np.asarray(region, np.float64).reshape(-1, 4)
    u = np.asarray(u, np.float64).reshape(-1, 2)
    return np.stack([region[:, 0] + (region[:, 1] - region[:, 0]) * u[:, 0],
                     region[:, 2] + (region[:, 3] - region[:, 2]) * u[:, 1]], 1)


def cem_rollout(speed, angle, it, region, u, goal, a0=None, z=None, mean=None, std=None):
    """One CEM iteration of n problems x P paths x T steps: every path starts at
    region_sample(region, u); iteration 0 takes a0 [n][P][T][2], later ones
    f64(mean) + f64(std) * z (mean, std [n][T][2] float32, z [n][P][T][2]). Returns
    (actions [n][P][T][2] float32, unclipped; paths [n][P][T+1][2] f64, free running;
    paths32 = float32(paths); reward [n][P])."""
    if it == 0:
        a = np.asarray(a0, np.float64)
    else:
        assert mean.dtype == std.dtype == np.float32
        a = (mean.astype(np.float64)[:, None] + std.astype(np.float64)[:, None]
             * np.asarray(z, np.float64))
    n, P, T = a.shape[:3]
    start = np.repeat(region_sample(region, u), P, 0)
    paths, _ = rollout(speed, angle, start, a.reshape(n * P, T, 2))
    paths = paths.reshape(n, P, T + 1, 2)
    goal = np.asarray(goal, np.float64).reshape(n, 2)
    reward = path_reward(paths[:, :, T].reshape(-1, 2), np.repeat(goal, P, 0)).reshape(n, P)
    return a.astype(np.float32), paths, paths.astype(np.float32), reward


def elite_order(reward):
    """Ascending reward, ties by path index, as an explicit rank count: order[rank[p]] = p with
    rank[p] = #{q : r[q] < r[p] or (r[q] == r[p] and q < p)}."""
    r = np.asarray(reward, np.float64)
    P = len(r)
    p, q = np.arange(P)[:, None], np.arange(P)[None, :]
    rank = ((r[q] < r[p]) | ((r[q] == r[p]) & (q < p))).sum(1)
    order = np.full(P, -1, np.int64)
    order[rank] = np.arange(P)
    assert (order >= 0).all()
    return order


def elite(reward, actions, E):
    """environment.py:166-173 for one problem: reward [P], actions [P][T][2] float32. The elites
    are the last E of elite_order; mean and std are numpy's float32 reductions over them written
    out: a sequential sum in elite order, / f32(E); (x - mu)^2 summed the same way, / f32(E), sqrt.
    Returns (order [P], mean [T][2] f32, std [T][2] f32, best = first maximum)."""
    actions = np.asarray(actions)
    assert actions.dtype == np.float32
    order = elite_order(reward)
    el = order[len(order) - E:]
    n = np.float32(E)
    total = actions[el[0]].copy()
    for e in el[1:]:
        total = total + actions[e]
    mu = total / n
    d = actions[el[0]] - mu
    sq = d * d
    for e in el[1:]:
        d = actions[e] - mu
        sq = sq + d * d
    sd = np.sqrt(sq / n)
    assert mu.dtype == sd.dtype == np.float32
    r = np.asarray(reward, np.float64)
    best = 0
    for q in range(1, len(r)):
        if r[q] > r[best]:
            best = q
    return order, mu, sd, best


def tie_patterns(P_, E_, rng):
    """The tied-reward cases the elite tests plant, name -> rewards [P_] in a shuffled path order
    (negative f64 but for the signed zeros): two elites tied, ranks P-E-1 and P-E tied (the
    cutoff), three tied across the cutoff, all equal, the maximum reached twice, -0.0 against 0.0.
    Cases a (P_, E_) has no room for are left out."""
    base = -np.sort(rng.uniform(1, 100, P_))[::-1]      # ascending, distinct
    perm = rng.permutation(P_)

    def shuffled(sorted_r):
        r = np.empty(P_)
        r[perm] = sorted_r
        return r

    out = {"distinct": shuffled(base)}
    if E_ >= 2:
        s = base.copy()
        s[P_ - 1] = s[P_ - 2]
        out["two_elites_tied"] = shuffled(s)
    if E_ < P_:
        s = base.copy()
        s[P_ - E_ - 1] = s[P_ - E_]
        out["cutoff_tied"] = shuffled(s)
    if E_ < P_ and P_ >= 3:
        s = base.copy()
        s[P_ - E_ - 1] = s[P_ - E_ + 1 if E_ >= 2 else P_ - E_ - 2] = s[P_ - E_]
        out["three_across_cutoff"] = shuffled(s)
    out["all_equal"] = np.full(P_, -3.25)
    s = base.copy()
    s[P_ - 1] = s[P_ - 2] if P_ > 1 else s[P_ - 1]
    out["max_twice"] = shuffled(s)
    s = base.copy()
    s[-1] = 0.0
    if P_ > 1:
        s[-2] = -0.0
    out["signed_zero"] = shuffled(s)
    s = base.copy()
    s[-1] = -0.0
    if P_ > 1:
        s[-2] = 0.0
    out["signed_zero_swapped"] = shuffled(s)
    return out


def demonstrations(speed, angle, regions, goals, uniforms, a0, z, E):
    """get_demonstration for n problems: regions [n][4], goals [n][2], uniforms [n][2],
    a0 [n][P][T][2], z [n][I-1][P][T][2]. Returns a dict with every iteration's actions
    [I][n][P][T][2] f32, paths [I][n][P][T+1][2] f64 and paths32 (float32 of them), reward
    [I][n][P], order [I][n][P], mean / std [I][n][T][2] f32, best [I][n], and the plan
    (environment.py:173-179): states [n][T][2] f32 = the last iteration's best path without its
    final state, plan_actions [n][T][2] f32."""
    a0 = np.asarray(a0, np.float64)
    z = np.asarray(z, np.float64)
    n, P, T = a0.shape[:3]
    I = z.shape[1] + 1
    out = {k: [] for k in ("actions", "paths", "paths32", "reward", "order", "mean", "std", "best")}
    mean = std = None
    for it in range(I):
        act, paths, p32, rew = cem_rollout(speed, angle, it, regions, uniforms, goals, a0=a0,
                                           z=z[:, it - 1] if it else None, mean=mean, std=std)
        el = [elite(rew[k], act[k], E) for k in range(n)]
        mean = np.stack([e[1] for e in el])
        std = np.stack([e[2] for e in el])
        for k, v in zip(out, (act, paths, p32, rew, np.stack([e[0] for e in el]), mean, std,
                              np.array([e[3] for e in el]))):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    ar = np.arange(n)
    out["states"] = out["paths32"][-1][ar, out["best"][-1], :T]
    out["plan_actions"] = out["actions"][-1][ar, out["best"][-1]]
    return out


def decisive_gaps(reward, E):
    """|r_e - r_q| of one problem's rewards [P] for every elite e (the last E of elite_order) and
    every path q, e itself excluded: the pairs whose order decides the elite set, the elites'
    summation order or best. Shape [E][P - 1]."""
    r = np.asarray(reward, np.float64)
    order = elite_order(r)
    return np.stack([np.abs(np.delete(r, e) - r[e]) for e in order[len(r) - E:]])


def assert_decisive_gaps(reward, E, bound=1e-4):
    """The precondition of a plan comparison, on the reference's rewards [I][n][P], no problem
    left out: any two rewards whose order can change the elites, their summation order or best
    are exactly equal or more than `bound` apart. A 1-ulp difference in a final float32 state
    moves a reward by at most sqrt(2) * 2^-17 = 1.1e-5 (the ulp of [64, 128))."""
    worst = np.inf
    for it in range(reward.shape[0]):
        for k in range(reward.shape[1]):
            g = decisive_gaps(reward[it, k], E)
            if (g > 0).any():
                worst = min(worst, float(g[g > 0].min()))
            assert np.all((g == 0) | (g > bound)), (it, k, float(g[g > 0].min()))
    print("smallest non-zero decisive reward gap", worst)


def augment_points(states, noise, steps, n_aug):
    """One demonstration's block of the demonstration set (robot.py:694-698 with the augmentation
    of robot.py:771-824; the layout of k_demo_augment): states [T][2] float32, noise
    [n_aug][(T-1)*(steps+1)*4 + 4] the augmentation's normal draws in the reference's order (per
    transition and sub-step: state 2, action 2; then the last state 2, last action 2). The T
    original states as f64, then per augmentation, for each transition i: `steps` interpolated
    states cur + f32((s+1)/(steps+1)) * (nxt - cur) in float32 plus their state noise, then cur
    plus noise; and finally the last state plus noise. [T + n_aug*((T-1)*(steps+1) + 1)][2] f64."""
    states = np.asarray(states)
    assert states.dtype == np.float32 and states.ndim == 2 and states.shape[1] == 2
    T = len(states)
    per = steps + 1
    D = (T - 1) * per * 4 + 4
    pts = [[np.float64(states[t, 0]), np.float64(states[t, 1])] for t in range(T)]
    for k in range(n_aug):
        g = np.asarray(noise[k], np.float64)
        assert g.shape == (D,)
        for i in range(T - 1):
            cur, nxt = states[i], states[i + 1]
            for s in range(per):
                gn = g[(i * per + s) * 4:(i * per + s) * 4 + 2]
                if s < steps:
                    f = np.float32(float(s + 1) / float(steps + 1))
                    b = [cur[c] + f * (nxt[c] - cur[c]) for c in range(2)]
                    assert all(type(v) is np.float32 for v in b)
                else:
                    b = [cur[0], cur[1]]
                pts.append([np.float64(b[0]) + gn[0], np.float64(b[1]) + gn[1]])
        last = states[T - 1]
        pts.append([np.float64(last[0]) + g[D - 4], np.float64(last[1]) + g[D - 3]])
    return np.array(pts, np.float64).reshape(-1, 2)
