"""tests/cem_ref.py (the numpy restatement the CEM demonstrator kernels are held to by
tests/test_gpu_cem_kernels.py) pinned before anything on the GPU is compared with it: against the
reference's own demonstrations in the golden traces, against numpy's float32 mean / std and stable
argsort, and against nav.demos.augment."""
import numpy as np
import pytest

import cem_ref
from conftest import golden
from gpu_support import ulps_f32

TRACES = ["trace.npz", "trace_branches.npz", "trace_branches_field.npz"]
P, T, I, E = 100, 200, 4, 10   # environment.py's CEM constants


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(orc):
    return orc


def consume_init_and_goal(rs):
    """environment.py:28-56 on RandomState rs: (region, goal), its draws consumed."""
    r = rs.choice([0, 1, 2, 3])
    S, W = 25, 100
    v = rs.uniform(0, W - S)
    if r == 0:
        l, rr, b, t = 0, S, v, v + S
    elif r == 1:
        l, rr, b, t = v, v + S, W - S, W
    elif r == 2:
        l, rr, b, t = W - S, W, v, v + S
    else:
        l, rr, b, t = v, v + S, 0, S
    mid = np.array([0.5 * (l + rr), 0.5 * (b + t)])
    dist = 0
    while dist < 90:
        goal = rs.uniform(5, W - 5, 2)
        dist = np.linalg.norm(goal - mid)
    return np.array([l, rr, b, t], np.float64), goal


_golden_runs = {}


def golden_run(name):
    """cem_ref.demonstrations on the trace's own stream: seeded as test_gpu_dropin's _trace_setup,
    set_init_and_goal's and the reset's draws consumed, then the 3 demonstrations' draws."""
    if name not in _golden_runs:
        from nav.cem import group_stream_draws
        t = golden(name)
        rs = np.random.RandomState(int(t["seed"]) if "seed" in t.files else 1707366464)
        region, goal = consume_init_and_goal(rs)
        rs.random_sample(2)  # env.reset()
        draws = group_stream_draws(rs, n_demos=3)
        n = len(draws)
        out = cem_ref.demonstrations(
            t["speed"], t["angle"], np.tile(region, (n, 1)), np.tile(goal, (n, 1)),
            np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws]),
            np.stack([d[2] for d in draws]), E)
        _golden_runs[name] = (t, region, goal, out)
    return _golden_runs[name]


@pytest.mark.parametrize("name", TRACES)
def test_restatement_reproduces_golden_demonstrations(name):
    t, region, goal, out = golden_run(name)
    assert np.array_equal(goal, t["goal"])
    assert np.array_equal(region, t["region"])
    assert t["demo_actions"].shape == (3, T, 2) and out["actions"].shape == (I, 3, P, T, 2)
    for k in range(3):
        assert out["plan_actions"][k].dtype == np.float32
        assert np.array_equal(out["plan_actions"][k], t["demo_actions"][k]), k
        u = ulps_f32(out["states"][k], t["demo_states"][k])
        print(name, k, "state ulps", int(u.max()))
        assert u.max() <= 1, (k, int(u.max()))


def test_goldens_contain_tied_rewards():
    """The tie rule is not hypothetical: the goldens' CEM iterations hold exactly tied rewards
    (paths clamped into one corner, float32 rounding of the final state)."""
    tied = {}
    for name in TRACES:
        rew = golden_run(name)[3]["reward"]            # [I][3][P]
        tied[name] = sum(len(np.unique(r)) < len(r) for r in rew.reshape(-1, P))
    print(tied)
    assert tied["trace_branches.npz"] >= 1
    assert sum(tied.values()) >= 1


@pytest.mark.parametrize("E_", [1, 2, 10, 100, 256])
def test_sequential_float32_mean_std_equal_numpy(E_):
    rng = np.random.default_rng(E_)
    P_ = max(E_, 7) + (3 if E_ < 256 else 0)
    act = (rng.standard_normal((P_, 5, 2)) * 3).astype(np.float32)
    rew = -rng.uniform(1, 100, P_)
    order, mu, sd, best = cem_ref.elite(rew, act, E_)
    idx = np.argsort(rew, kind="stable")[-E_:]
    assert np.array_equal(order[-E_:], idx)
    sel = act[idx]
    assert sel.dtype == np.float32 and sel.shape == (E_, 5, 2)
    assert np.array_equal(mu, np.mean(sel, axis=0))
    assert np.array_equal(sd, np.std(sel, axis=0))
    assert best == np.argmax(rew)


@pytest.mark.parametrize("P_,E_", [(1, 1), (9, 1), (9, 3), (9, 9), (100, 10), (256, 10)])
def test_elite_order_is_stable_argsort(P_, E_):
    rng = np.random.default_rng(100 * P_ + E_)
    act = (rng.standard_normal((P_, 3, 2)) * 3).astype(np.float32)
    for name, rew in cem_ref.tie_patterns(P_, E_, rng).items():
        order, mu, sd, best = cem_ref.elite(rew, act, E_)
        want = np.argsort(rew, kind="stable")
        assert np.array_equal(order, want), name
        assert best == np.argmax(rew), name
        sel = act[want[-E_:]]
        assert np.array_equal(mu, np.mean(sel, axis=0)), name
        assert np.array_equal(sd, np.std(sel, axis=0)), name


@pytest.mark.parametrize("T_", [2, 5, 200])
def test_augment_points_equal_nav_augment(T_):
    from nav import config as K
    from nav.demos import augment, augment_draws
    rng = np.random.default_rng(T_)
    st = rng.uniform(0, 98.9, (T_, 2)).astype(np.float32)
    ac = rng.uniform(-5, 5, (T_, 2)).astype(np.float32)
    draws = augment_draws(np.random.RandomState(T_), T_)
    want = np.concatenate([st.astype(np.float64)] + [s for s, _ in augment(st, ac, draws=draws)])
    got = cem_ref.augment_points(st, np.stack(draws), K.AUG_INTERPOLATION, K.NUM_AUGMENTS)
    assert got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want)


@pytest.mark.parametrize("steps,n_aug", [(0, 1), (2, 0), (0, 0), (1, 2)])
def test_augment_points_degenerate_shapes(steps, n_aug):
    """steps = 0 and n_aug = 0, which nav.demos.augment cannot form: the block's size and its
    un-interpolated rows follow from the definition."""
    T_ = 4
    rng = np.random.default_rng(7)
    st = rng.uniform(0, 98.9, (T_, 2)).astype(np.float32)
    D = (T_ - 1) * (steps + 1) * 4 + 4
    noise = rng.normal(0, 0.1, (n_aug, D))
    got = cem_ref.augment_points(st, noise, steps, n_aug)
    A = (T_ - 1) * (steps + 1) + 1
    assert got.shape == (T_ + n_aug * A, 2)
    assert np.array_equal(got[:T_], st.astype(np.float64))
    for k in range(n_aug):
        blk = got[T_ + k * A:T_ + (k + 1) * A]
        body = noise[k, :-4].reshape(T_ - 1, steps + 1, 4)
        # the sub-step `steps` of every transition is the current state plus its noise
        assert np.array_equal(blk[steps:A - 1:steps + 1], st[:-1].astype(np.float64)
                              + body[:, steps, :2])
        assert np.array_equal(blk[-1], st[-1].astype(np.float64) + noise[k, -4:-2])
