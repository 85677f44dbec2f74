"""The oracle's batched entry points against its own per-env / per-draw forms. CPU only.

The GPU tests compare whole launches (65 536 envs, 16 421-row batches) with the oracle through
VecAgentState.step_batch and the batched restatements of the product path's three in-kernel Philox
streams (exploration noise, replay indices, target-smoothing noise). Here those are pinned to the
per-env tick that the golden trace pins to the reference (test_oracle_golden.py) and to the stream
formulas evaluated one draw at a time through oracle.philox."""
import math

import numpy as np
import pytest

from conftest import golden

FIELDS = ("state", "goal", "region", "hist", "meta", "plan_index", "path_length", "episodes",
          "noise_scale")
SEED = (0x5A17 << 32) | 424242  # seed_hi != 0


def _mirror(orc, p, n, epg):
    """n envs in groups of epg as nav_env_init leaves them (init draw per group, reset draw per
    env), then crafted so that 25 ticks reach every branch: the homing quarter starts 6 units
    from its goal, and every third env has a short path (its plan ends at tick 10)."""
    st = orc.VecAgentState(n)
    for e in range(n):
        st.region[e], st.goal[e], _ = orc.vec_init_one(p, e // epg)
        st.state[e] = orc.vec_reset_one(p, e, 5, st.region[e])
    st.plan_index[:] = 5
    st.path_length[:] = 50
    st.path_length[::3] = 16
    st.episodes[:] = 5
    st.noise_scale[:] = 1.0
    st.meta[:] = 4  # demo_flag
    d = st.state[: n // 4] - st.goal[: n // 4]
    st.state[: n // 4] = st.goal[: n // 4] + 6.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return st


def _clone(orc, st):
    out = orc.VecAgentState(st.n)
    for k in FIELDS:
        getattr(out, k)[:] = getattr(st, k)
    return out


@pytest.mark.parametrize("indexed", [False, True])
def test_step_batch_equals_per_env_ticks(orc, indexed):
    """VecAgentState.step_batch, one call per demo group over [lo, hi) of the mirror, equals
    VecAgentState.tick env by env, bit for bit: replay rows, next_state, flags, rewards and every
    field of the mirror, for 25 ticks of 300 envs in 3 groups (each with its own demo set) under
    the action mix of test_agent_step_vs_oracle_per_step (a quarter homing, a quarter near zero,
    the rest uniform in +-6), brute-force and through the exact demo index."""
    g = golden("trace.npz")
    speed, angle, demo = g["speed"], g["angle"], g["demo_set"]
    n, epg, steps = 300, 100, 25
    G = n // epg
    sets = [np.ascontiguousarray(demo + 0.5 * k) for k in range(G)]
    index = [orc.DemoIndexCPU(s) if indexed else None for s in sets]
    p = orc.default_params(SEED)
    one = _mirror(orc, p, n, epg)
    many = _clone(orc, one)
    cap = 3 * n + 7  # the ring wraps inside a group's range
    rows_one = np.zeros((cap, 8), np.float32)
    rows_many = np.zeros((cap, 8), np.float32)
    rng = np.random.default_rng(0)
    seen = dict(done=0, goal=0, stuck=0, ended=0, demo_term=0)
    base = 0
    for t in range(steps):
        a = rng.uniform(-6, 6, (n, 2))
        a[: n // 4] = np.clip(one.goal[: n // 4] - one.state[: n // 4], -5, 5)
        a[n // 4: n // 2] = rng.uniform(-0.05, 0.05, (n // 4, 2))
        fl_one = np.zeros(n, np.int32); ns_one = np.zeros((n, 2)); r_one = np.zeros(n)
        for e in range(n):
            fl_one[e], ns_one[e], row, r_one[e] = one.tick(p, speed, angle, sets[e // epg], e, a[e])
            rows_one[(base + e) % cap] = row
        for k in range(G):
            lo, hi = k * epg, (k + 1) * epg
            ns, fl, r = many.step_batch(p, speed, angle, sets[k], a, rows_many, base, lo, hi,
                                        index=index[k])
            assert np.array_equal(ns, ns_one[lo:hi]), (t, k)
            assert np.array_equal(fl, fl_one[lo:hi]), (t, k)
            assert np.array_equal(r, r_one[lo:hi]), (t, k)
        for f in FIELDS:
            assert np.array_equal(getattr(many, f), getattr(one, f)), (t, f)
        assert np.array_equal(rows_many, rows_one), t
        base = (base + n) % cap
        for bit, key in enumerate(("done", "goal", "stuck", "ended")):
            seen[key] += int(((fl_one >> bit) & 1).sum())
        # the demo term is part of every reward of a demo_flag env that did not reach its goal
        seen["demo_term"] += int((((fl_one & 2) == 0) & ((one.meta & 4) != 0)).sum())
    assert all(v > 0 for v in seen.values()), seen
    assert (one.episodes > 5).any() and (one.noise_scale < 1.0).any()


def test_step_batch_range_leaves_other_envs_alone(orc):
    g = golden("trace.npz")
    p = orc.default_params(SEED)
    st = _mirror(orc, p, 40, 10)
    before = _clone(orc, st)
    rows = np.full((64, 8), np.nan, np.float32)
    a = np.random.default_rng(1).uniform(-5, 5, (40, 2))
    ns, fl, r = st.step_batch(p, g["speed"], g["angle"], g["demo_set"], a, rows, 50, 10, 20)
    assert ns.shape == (10, 2) and fl.shape == (10,) and r.shape == (10,)
    for f in FIELDS:
        x, y = getattr(st, f), getattr(before, f)
        assert np.array_equal(x[:10], y[:10]) and np.array_equal(x[20:], y[20:]), f
    written = ~np.isnan(rows[:, 0])
    assert np.array_equal(np.nonzero(written)[0], np.sort((50 + np.arange(10, 20)) % 64))
    assert np.array_equal(rows[(50 + 10) % 64, 2:4], a[10].astype(np.float32))


def _gauss_pair(w):
    """nav_device.h:93-98 from four Philox words, in Python floats (libm, as the oracle)."""
    u01 = lambda hi, lo: ((hi >> 5) * 67108864.0 + (lo >> 6)) / 9007199254740992.0  # noqa: E731
    u1, u2 = u01(w[0], w[1]), u01(w[2], w[3])
    rad = math.sqrt(-2.0 * math.log(1.0 - u1))
    th = 6.283185307179586 * u2
    return rad * math.cos(th), rad * math.sin(th)


def test_vec_noise_equals_vec_noise_one(orc):
    p = orc.default_params(SEED)
    key = (p.seed_lo, p.seed_hi)
    for step in (0, 7, 0xFFFFFFFF):
        z = orc.vec_noise(p, 777, step)
        assert z.shape == (777, 2) and z.dtype == np.float64
        for e in range(777):
            assert np.array_equal(z[e], orc.vec_noise_one(p, e, step)), (step, e)
        for e in (0, 1, 500, 776):  # ctr = (0, env, NAV_TAG_NOISE, step)
            assert tuple(z[e]) == _gauss_pair(orc.philox((0, e, 3, step), key)), (step, e)


def test_sample_indices_formula_and_range(orc):
    p = orc.default_params(SEED)
    key = (p.seed_lo, p.seed_hi)
    B = 2000
    for size in (1, 1000, 2 ** 31 - 1):
        for ctr in (0, 11, 0xFFFFFFFF):
            idx = orc.sample_indices(p, B, size, ctr)
            assert idx.shape == (B,) and idx.dtype == np.int64
            assert idx.min() >= 0 and idx.max() < size
            ref = [(orc.philox((b, 0, 4, ctr), key)[0] * size) >> 32 for b in range(B)]
            assert idx.tolist() == ref, (size, ctr)
    assert (orc.sample_indices(p, B, 1, 3) == 0).all()
    # the draw covers the fill it is given, not a fixed capacity
    assert orc.sample_indices(p, B, 2 ** 31 - 1, 3).max() > 2 ** 30


def test_smoothing_noise_formula(orc):
    p = orc.default_params(SEED)
    key = (p.seed_lo, p.seed_hi)
    for ctr in (0, 5, 0xFFFFFFFF):
        eps = orc.smoothing_noise(p, 1500, ctr)
        assert eps.shape == (1500, 2) and eps.dtype == np.float32
        for r in range(1500):  # ctr = (row, 0, NAV_TAG_TNOISE, ctr), rounded to f32
            want = np.array(_gauss_pair(orc.philox((r, 0, 5, ctr), key)), np.float64)
            assert np.array_equal(eps[r], want.astype(np.float32)), (ctr, r)


def test_streams_are_distinct(orc):
    """The three streams differ from each other and across the counter, the seed's high word
    changes every one, and the learner's counters never meet: an epoch's critic batch, its actor
    batch and the next epoch's are three different draws."""
    p = orc.default_params(SEED)
    q = orc.default_params(SEED & 0xFFFFFFFF)  # seed_hi dropped
    assert p.seed_lo == q.seed_lo and p.seed_hi != 0 and q.seed_hi == 0
    n, c = 4096, 6
    full = 2 ** 32  # size 2^32: the index is the first Philox word itself
    draws = {
        "noise": orc.vec_noise(p, n, c).astype(np.float32),
        "smooth": orc.smoothing_noise(p, n, c),
        "noise+1": orc.vec_noise(p, n, c + 1).astype(np.float32),
        "smooth+1": orc.smoothing_noise(p, n, c + 1),
        "noise_hi0": orc.vec_noise(q, n, c).astype(np.float32),
        "smooth_hi0": orc.smoothing_noise(q, n, c),
    }
    names = list(draws)
    for i, a in enumerate(names):
        assert np.isfinite(draws[a]).all()
        assert abs(draws[a].mean()) < 5 / math.sqrt(2 * n) and abs(draws[a].std() - 1) < 0.1
        for b in names[i + 1:]:
            assert (draws[a] == draws[b]).mean() < 0.001, (a, b)
            assert abs(np.corrcoef(draws[a].ravel(), draws[b].ravel())[0, 1]) < 5 / math.sqrt(
                2 * n), (a, b)
    words = {
        "sample": orc.sample_indices(p, n, full, c),
        "sample+1": orc.sample_indices(p, n, full, c + 1),
        "sample_hi0": orc.sample_indices(q, n, full, c),
        # the first word of the other two streams' counters for the same (row, counter)
        "noise_word": np.array([orc.philox((0, b, 3, c), (p.seed_lo, p.seed_hi))[0]
                                for b in range(n)], np.int64),
        "smooth_word": np.array([orc.philox((b, 0, 5, c), (p.seed_lo, p.seed_hi))[0]
                                 for b in range(n)], np.int64),
    }
    names = list(words)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (words[a] == words[b]).mean() < 0.001, (a, b)
    ctrs = [orc.learner_counters(u) for u in range(200)]
    for u, k in enumerate(ctrs):
        assert k == {"critic_sample": 2 * u, "actor_sample": 2 * u + 1, "smoothing": u}
    samples = [k[w] for k in ctrs for w in ("critic_sample", "actor_sample")]
    assert len(set(samples)) == len(samples)
    assert orc.learner_counters(0x80000003) == {"critic_sample": 6, "actor_sample": 7,
                                                "smoothing": 0x80000003}  # uint32, as the launcher
