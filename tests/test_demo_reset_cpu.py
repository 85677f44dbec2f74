"""Resets to demonstration states, host side: the `usable` table on a hand-made set, the
restatement tests/demo_reset_ref.py pinned by hand-worked values and by its own statistics on
65 536 reset envs, the argument sets nav_demo_reset refuses with the raw status NAV_EINVAL before
any HIP call (no kernel is launched, the dummy pointers are never followed, so no GPU is needed),
and the refusals and the routing of the trainer and the population that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import demo_reset_ref as D
from abi_args import EINVAL, F, Call, load_raw
from abi_args import v as _v

SEED = 1707366464
NAN = float("nan")


# ---- the usable table
def hand_set():
    """Three demonstrations of T = 7 states walking along x towards the goal (50, 50), threshold 5:
    one enters the goal disc at index 3, one never does, one starts inside."""
    T = 7
    xs = np.array([[20, 30, 40, 46, 48, 50, 50],      # |x - 50| = 30 20 10 4 ...: inside from 3
                   [0, 5, 10, 15, 20, 25, 30],        # never within 5
                   [47, 40, 30, 20, 10, 5, 0]],       # starts inside (3 away)
                  np.float32)
    states = np.stack([xs, np.full_like(xs, 50.0)], -1)
    assert states.shape == (3, T, 2)
    goals = np.full((3, 2), 50.0)
    return states, goals


def test_usable_on_a_hand_made_set():
    from nav.demos import demo_reset_usable
    states, goals = hand_set()
    got = demo_reset_usable(states, goals, 5.0)
    assert got.dtype == np.int32 and got.tolist() == [3, 6, 1]  # 6 = T - 1: never the last state
    assert D.usable(states, goals, 5.0).tolist() == [3, 6, 1]
    # exactly on the disc's edge counts as inside (the tick's goal test is <=)
    edge = states.copy()
    edge[0, 2, 0] = 45.0
    assert demo_reset_usable(edge, goals, 5.0).tolist() == [2, 6, 1]
    assert D.usable(edge, goals, 5.0).tolist() == [2, 6, 1]
    # a demonstration that leaves the disc again: only the leading states count
    back = states.copy()
    back[0, 4:, 0] = 10.0
    assert demo_reset_usable(back, goals, 5.0).tolist() == [3, 6, 1]
    # each demonstration against its own goal, and the threshold is the caller's
    far = goals.copy()
    far[0] = (0.0, 0.0)
    assert demo_reset_usable(states, far, 5.0).tolist() == [6, 6, 1]
    assert demo_reset_usable(states, goals, 11.0).tolist() == [2, 6, 1]
    # random sets: the vectorised table is the loop's
    rng = np.random.default_rng(1)
    st = (rng.random((40, 9, 2)) * 30).astype(np.float32)
    gl = rng.random((40, 2)) * 30
    got = demo_reset_usable(st, gl, 5.0)
    assert np.array_equal(got, D.usable(st, gl, 5.0))
    assert got.min() >= 1 and got.max() <= 8 and len(set(got.tolist())) > 3


# ---- the restatement's pieces, by hand
def test_u01_and_mulhi_by_hand():
    assert D.u01(0, 0) == 0.0
    assert D.u01(0x80000000, 0) == 0.5
    assert D.u01(0x20, 0x40) == (2.0 ** 26 + 1) / 2.0 ** 53  # the 27 + 26 bits that are used
    assert D.u01(0x1F, 0x3F) == 0.0                          # the 5 + 6 low bits are dropped
    assert D.u01(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 < 1.0
    assert D.u01(0x40000000, 0) == 0.25 and not D.u01(0x40000000, 0) < 0.25
    assert D.u01(0x3FFFFFFF, 0xFFFFFFFF) < 0.25
    assert D.mulhi(0xFFFFFFFF, 3) == 2 and D.mulhi(0, 3) == 0
    assert D.mulhi(0x55555555, 3) == 0 and D.mulhi(0x55555556, 3) == 1
    assert D.mulhi(0xAAAAAAAA, 3) == 1 and D.mulhi(0xAAAAAAAB, 3) == 2
    assert D.mulhi(0x80000000, 7) == 3 and D.mulhi(0xFFFFFFFF, 1) == 0
    assert D.NAV_TAG_DRESET == 9


def test_the_draw_is_keyed_by_env_episode_and_seed():
    a = D.draw(5, 7, SEED)
    assert a == D.draw(5, 7, SEED) and len(a) == 4 and all(0 <= w < 2 ** 32 for w in a)
    assert len({tuple(D.draw(*k)) for k in ((5, 7, SEED), (6, 7, SEED), (5, 8, SEED),
                                            (5, 7, SEED + 1), (5, 7, SEED + (1 << 32)))}) == 5
    # the tag keeps the stream apart from the tick's own reset draw (NAV_TAG_RESET = 2)
    from oracle import oracle as O
    assert a != [int(x) for x in O.philox((0, 5, 2, 7), (SEED & 0xFFFFFFFF, SEED >> 32))]


# ---- the restatement alone
@pytest.fixture(scope="module")
def big():
    """65 536 reset envs in one group at prob 0.25, n_demos 3, usable (1, 4, 6), T = 7."""
    n, T = 65536, 7
    demo = np.zeros((3, T, 2), np.float32)
    for d in range(3):
        for t in range(T):
            demo[d, t] = (100 + 10 * d + t, -(100 + 10 * d + t))
    state = np.zeros((n, 2))
    flags = np.full(n, 8, np.uint8)
    episodes = np.full(n, 6, np.int32)
    new, counts, picks = D.reset(state, flags, episodes, SEED, demo, (1, 4, 6), 3, n, 0.25)
    return dict(n=n, demo=demo, new=new, counts=counts, picks=picks)


def test_reference_share_and_cells(big):
    n, picks = big["n"], big["picks"]
    took = picks[:, 0] >= 0
    share = took.mean()
    sd = math.sqrt(0.25 * 0.75 / n)
    print(f"share {share:.5f}, 0.25 +- {4 * sd:.5f}")
    assert abs(share - 0.25) <= 4 * sd
    assert big["counts"].sum() == took.sum() and big["counts"].shape == (n // 64,)
    assert np.array_equal(big["counts"], took.reshape(-1, 64).sum(1))
    cells = {(int(d), int(t)) for d, t in picks[took]}
    assert cells == {(d, t) for d, u in enumerate((1, 4, 6)) for t in range(u)}
    # the state is the cell's, as f64 of the f32; the others keep theirs
    d, t = picks[took].T
    assert np.array_equal(big["new"][took], big["demo"][d, t].astype(np.float64))
    assert (big["new"][~took] == 0).all()


def test_reference_touches_only_flagged_envs_and_follows_prob_group():
    rng = np.random.default_rng(2)
    n, epg, T = 200, 64, 7
    demo = rng.random((4 * 3, T, 2)).astype(np.float32) + 1
    us = rng.integers(1, T, 12)
    flags = rng.integers(0, 256, n).astype(np.uint8)
    ep = rng.integers(5, 1 << 20, n).astype(np.int32)
    state = np.zeros((n, 2))
    new, counts, picks = D.reset(state, flags, ep, SEED, demo, us, 3, epg, 1.0)
    took = picks[:, 0] >= 0
    assert np.array_equal(took, (flags & 8) != 0) and counts.tolist() == [
        int(took[k:k + 64].sum()) for k in range(0, n, 64)]
    g = np.arange(n) // epg
    j = g[took] * 3 + picks[took, 0]
    assert (picks[took, 1] < us[j]).all()
    assert np.array_equal(new[took], demo[j, picks[took, 1]].astype(np.float64))
    # per group: 0 never, 1 always, and prob is then not looked at
    new, counts, picks = D.reset(state, flags, ep, SEED, demo, us, 3, epg, 1.0, (0, 1, 0.5, 0.25))
    took = picks[:, 0] >= 0
    flagged = (flags & 8) != 0
    assert not took[g == 0].any() and np.array_equal(took[g == 1], flagged[g == 1])
    assert 0 < took[g == 2].sum() < flagged[g == 2].sum()


# ---- the entry point's host-side refusals
@pytest.fixture(scope="module")
def raw():
    return load_raw()


def env(n=200, state=F, episodes=F):
    from nav._lib import NavEnvSoa
    fields = [F] * 9
    fields[0], fields[7] = state, episodes
    return lambda: C.byref(NavEnvSoa(n, *fields))


CALL = Call("nav_demo_reset", env=env(), flags=_v(F), seed_lo=_v(1), seed_hi=_v(2),
            demo_states=_v(F), usable=_v(F), n_demos=_v(3), T=_v(7), envs_per_group=_v(64),
            prob=_v(0.25), prob_group=_v(None), counts=_v(None), stream=_v(None))
CALLS = {CALL.fn: CALL}

BAD = [("nav_demo_reset", what, changed) for what, changed in (
    ("no env", dict(env=_v(None))),
    ("no flags", dict(flags=_v(None))),
    ("no demo_states", dict(demo_states=_v(None))),
    ("no usable", dict(usable=_v(None))),
    ("n_demos = 0", dict(n_demos=_v(0))),
    ("n_demos < 0", dict(n_demos=_v(-3))),
    ("T = 1", dict(T=_v(1))),
    ("T = 0", dict(T=_v(0))),
    ("envs_per_group = 0", dict(envs_per_group=_v(0))),
    ("envs_per_group < 0", dict(envs_per_group=_v(-64))),
    ("prob < 0", dict(prob=_v(-0.01))),
    ("prob > 1", dict(prob=_v(1.0000001))),
    ("prob NaN", dict(prob=_v(NAN))),
    ("prob inf", dict(prob=_v(float("inf")))),
    ("n < 0", dict(env=env(-1))),
    ("n = 2^31", dict(env=env(1 << 31))),
    ("no env.state", dict(env=env(state=None))),
    ("no env.episodes", dict(env=env(episodes=None))),
    # a refusal comes before the empty set's return
    ("no flags and no envs", dict(flags=_v(None), env=env(0))),
    ("prob NaN and no envs", dict(prob=_v(NAN), env=env(0))),
)]


@pytest.mark.parametrize("fn,what,changed", BAD, ids=[b[1] for b in BAD])
def test_bad_arguments_return_einval(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == EINVAL


def test_no_envs_is_no_launch(raw):
    assert CALL(raw, env=env(0)) == 0
    assert CALL(raw, env=env(0, state=None, episodes=None), prob=_v(1.0)) == 0
    assert CALL(raw, env=env(0), prob=_v(0.0), prob_group=_v(F), counts=_v(F)) == 0


def test_header_binding_and_tag():
    import os
    import re
    from conftest import ROOT
    from nav._lib import SIGNATURES
    sig = {s[0]: s for s in SIGNATURES}["nav_demo_reset"]
    assert sig[1] is C.c_int and len(sig[2]) == 13 and sig[2][9] is C.c_double
    src = open(os.path.join(ROOT, "include", "navenv.h")).read()
    assert re.search(r"#define NAV_TAG_DRESET 9\b", src)
    assert re.search(r"#define NAV_ABI_VERSION 11\b", src)


# ---- the trainer and the population, before any device work
@pytest.fixture
def no_device(monkeypatch):
    """Whatever a constructor does first on the device raises AssertionError: a ValueError that
    arrives all the same was raised before it, on any machine."""
    import nav.mlp
    import nav.population
    import nav.trainer

    def touched(*a, **kw):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(nav.trainer, "make_field_device", touched)
    monkeypatch.setattr(nav.trainer, "make_env", touched)
    monkeypatch.setattr(nav.population, "make_field_device", touched)
    monkeypatch.setattr(nav.population, "make_env", touched)
    monkeypatch.setattr(nav.mlp.DeviceMLP, "__init__", touched)


@pytest.mark.parametrize("prob", [-0.1, 1.5, NAN, float("inf")])
def test_trainer_refuses_a_probability_outside_the_unit_interval(no_device, prob):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="demo_reset_prob"):
        VecTrainer(n_envs=256, hidden=64, batch=128, demo_reset_prob=prob)


def test_trainer_refuses_resets_without_demonstrations(no_device):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="demos=True"):
        VecTrainer(n_envs=256, hidden=64, batch=128, demos=False, demo_reset_prob=0.3)
    # a misspelt keyword is still no mode field
    with pytest.raises(TypeError, match="demo_reset_probability"):
        VecTrainer(n_envs=256, hidden=64, batch=128, demo_reset_probability=0.1)
    # 0 without demonstrations is the plain trainer: it gets as far as the device
    with pytest.raises(AssertionError, match="device work"):
        VecTrainer(n_envs=256, hidden=64, batch=128, demos=False, demo_reset_prob=0.0)


def test_it_is_no_learner_mode():
    from nav import config as K
    assert "demo_reset_prob" not in K.MODE_FIELDS
    assert not hasattr(K.TD3Config(), "demo_reset_prob")


def test_population_routing():
    from nav.population import (EXTRA_KEYS, PARAM_KEYS, PBT_ENV_KEYS, PBT_EXPLORE_KEYS,
                                PBT_OWN_KEYS, PBT_PARAM_KEYS, PBT_TD3_KEYS, TD3_KEYS, pbt_explore,
                                route_overrides)
    assert "demo_reset_prob" in EXTRA_KEYS and "demo_reset_prob" not in PARAM_KEYS | TD3_KEYS
    assert route_overrides({"demo_reset_prob": 0.3, "demo_factor": 30.0}) == (
        {"demo_factor": 30.0}, {}, {"demo_reset_prob": 0.3})
    assert PBT_ENV_KEYS == {"demo_reset_prob"} and PBT_ENV_KEYS <= PBT_EXPLORE_KEYS
    assert PBT_EXPLORE_KEYS == PBT_PARAM_KEYS | PBT_TD3_KEYS | PBT_ENV_KEYS
    assert "demo_reset_prob" not in PBT_PARAM_KEYS | PBT_TD3_KEYS | PBT_OWN_KEYS

    class Pick:
        def __init__(self, f):
            self.f = f

        def choice(self, options):
            return self.f
    assert pbt_explore({"demo_reset_prob": 0.4}, {"demo_reset_prob": (0.0, 1.0)},
                       Pick(1.25)) == {"demo_reset_prob": 0.5}
    assert pbt_explore({"demo_reset_prob": 0.9}, {"demo_reset_prob": (0.0, 1.0)},
                       Pick(1.25)) == {"demo_reset_prob": 1.0}


def test_population_refuses_before_it_builds(no_device):
    from nav.population import PopulationTrainer
    kw = dict(hidden=64, batch=64)
    with pytest.raises(ValueError, match="whole env groups"):
        PopulationTrainer([{}, {"demo_reset_prob": 0.3}], envs_per_member=64, envs_per_group=128,
                          **kw)
    with pytest.raises(ValueError, match="demos=True"):
        PopulationTrainer([{}, {"demo_reset_prob": 0.3}], envs_per_member=64, envs_per_group=64,
                          demos=False, **kw)
    with pytest.raises(ValueError, match=r"demo_reset_prob.*member 1"):
        PopulationTrainer([{}, {"demo_reset_prob": 1.5}], envs_per_member=64, envs_per_group=64,
                          **kw)
    # all zero: no whole-groups rule, the plain population (it gets as far as the device)
    with pytest.raises(AssertionError, match="device work"):
        PopulationTrainer([{}, {"demo_reset_prob": 0.0}], envs_per_member=64, envs_per_group=128,
                          demos=False, **kw)
