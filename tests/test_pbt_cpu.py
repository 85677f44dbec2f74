"""Population-based training, host side: the argument validation of nav_pop_test_summary,
nav_td3_pop_state_build and nav_td3_pop_exploit (every rejected condition returns NAV_EINVAL before
any HIP call and without following a pointer: no kernel is launched by these calls, so no GPU is
needed), the state table's size, and the pure selection and explore rules."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from abi_args import member_field as _member_field
from abi_args import net_field as _net_field
from abi_args import set_attr as _set
from abi_args import td3_member
from conftest import PKG

LIB = os.path.join(PKG, "nav", "libnavenv.so")
FAKE = 16  # a non-null, 16-byte-aligned pointer value that is never dereferenced on the host
P, CAP, H, NH = 4, 4096, 64, 3
EINVAL = -100000


@pytest.fixture(scope="module")
def navlib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib()


member = functools.partial(td3_member, hidden=H, n_hidden=NH, cap=CAP, state_only=True)


class Args:
    """A valid argument set of the state entry points; a case alters one thing."""

    def __init__(self, **kw):
        self.m = [member(**kw) for _ in range(P)]
        self.n, self.table = P, FAKE
        self.src, self.dst = [0, 0], [2, 3]
        self.n_pairs, self.rows = None, 3000

    def raw(self, L):
        from nav._lib import NavTd3Member
        a = (NavTd3Member * len(self.m))(*self.m)
        k = len(self.src) if self.n_pairs is None else self.n_pairs
        src, dst = (C.c_int32 * max(len(self.src), 1))(*self.src), \
            (C.c_int32 * max(len(self.dst), 1))(*self.dst)
        return {"build": lambda: L.raw.nav_td3_pop_state_build(a, self.n, self.table, None),
                "exploit": lambda: L.raw.nav_td3_pop_exploit(a, self.n, self.table, src, dst, k,
                                                             self.rows, None)}


def _pairs(src, dst):
    def f(a):
        a.src, a.dst = src, dst
    return f


BOTH, EXPLOIT = ("build", "exploit"), ("exploit",)
# (what is wrong, the change, the entry points that must refuse it)
BAD = [
    ("no members", _set("n", 0), BOTH),
    ("257 members", _set("n", 257), BOTH),
    ("no table", _set("table", None), BOTH),
    ("no pairs", _set("n_pairs", 0), EXPLOIT),
    ("as many pairs as members", _pairs([0, 0, 0, 0], [1, 2, 3, 1]), EXPLOIT),
    ("a population of one", lambda a: (_set("n", 1)(a), _pairs([0], [0])(a)), EXPLOIT),
    ("src index -1", _pairs([-1, 0], [2, 3]), EXPLOIT),
    ("src index n_members", _pairs([0, P], [2, 3]), EXPLOIT),
    ("dst index -1", _pairs([0, 0], [-1, 3]), EXPLOIT),
    ("dst index n_members", _pairs([0, 0], [2, P]), EXPLOIT),
    ("src == dst", _pairs([0, 3], [2, 3]), EXPLOIT),
    ("a repeated dst", _pairs([0, 1], [2, 2]), EXPLOIT),
    ("a dst that is also a src", _pairs([0, 2], [2, 3]), EXPLOIT),
    ("a src that was a dst", _pairs([0, 1], [1, 3]), EXPLOIT),
    ("another hidden width", _net_field("actor", "hidden", 32), BOTH),
    ("another padded width", _net_field("target_actor", "hidden_pad", 96), BOTH),
    ("another depth", _net_field("critics", "n_hidden", 2, 1), BOTH),
    ("another target depth", _net_field("target_critics", "n_hidden", 2, 0, m=3), BOTH),
    ("another ring capacity", lambda a: setattr(a.m[2].replay, "capacity", CAP // 2), BOTH),
    ("replay_rows = -1", _set("rows", -1), EXPLOIT),
    ("replay_rows = capacity + 1", _set("rows", CAP + 1), EXPLOIT),
    ("no actor params", _net_field("actor", "params", None), BOTH),
    ("no target critic image", _net_field("target_critics", "packed", None, 1), BOTH),
    ("no critic moment", _member_field("v_critic", None, 0), BOTH),
    ("no actor moment", _member_field("m_actor", None), BOTH),
    ("no ring rows", lambda a: setattr(a.m[1].replay, "rows", None), BOTH),
    ("params at 8 mod 16", _net_field("critics", "params", FAKE + 8, 0), BOTH),
    ("image at 8 mod 16", _net_field("actor", "packed", FAKE + 8, m=0), BOTH),
    ("moment at 8 mod 16", _member_field("m_critic", FAKE + 8, 1, m=3), BOTH),
    ("ring at 8 mod 16", lambda a: setattr(a.m[3].replay, "rows", FAKE + 8), BOTH),
]


# (the unaltered set launches: tests/test_gpu_pbt.py runs it on real buffers)
@pytest.mark.parametrize("what,change,entries", BAD, ids=[b[0] for b in BAD])
def test_bad_state_arguments_are_refused_on_the_host(navlib, what, change, entries):
    a = Args()
    change(a)
    calls = a.raw(navlib)
    for e in entries:
        assert calls[e]() == EINVAL, e


def test_one_hidden_layer_has_no_image(navlib):
    """n_hidden == 1: the packed segment is empty and its pointer is not looked at; the other
    rules still hold."""
    a = Args(hidden=32, n_hidden=1)
    for m in a.m:
        m.actor.packed = None
        m.critics[1].packed = FAKE + 8
    a.table = None  # the only thing wrong: refused for the table, not for the images
    assert all(f() == EINVAL for f in a.raw(navlib).values())
    b = Args(hidden=32, n_hidden=1)
    b.m[1].actor.params = None
    assert all(f() == EINVAL for f in b.raw(navlib).values())


def test_state_table_bytes(navlib):
    from nav._lib import NavError
    one = navlib.nav_td3_pop_state_bytes(1)
    assert one > 0 and one % 8 == 0
    for n in (2, 3, 256):
        assert navlib.nav_td3_pop_state_bytes(n) == n * one
    for bad in (0, -1, 257):
        with pytest.raises(NavError):
            navlib.nav_td3_pop_state_bytes(bad)
        assert navlib.raw.nav_td3_pop_state_bytes(bad) == EINVAL


SUMMARY_BAD = [("no members", dict(n=0)), ("257 members", dict(n=257)),
               ("no envs", dict(epm=0)), ("envs not a multiple of 64", dict(epm=96)),
               ("no reached", dict(reached=None)), ("no steps", dict(steps=None)),
               ("no best_distance", dict(best=None)), ("no scores", dict(scores=None)),
               ("no out", dict(out=False))]


@pytest.mark.parametrize("what,kw", SUMMARY_BAD, ids=[b[0] for b in SUMMARY_BAD])
def test_bad_summary_arguments_are_refused_on_the_host(navlib, what, kw):
    from nav._lib import NavError, NavTestOut
    v = dict(n=3, epm=192, reached=FAKE, steps=FAKE, best=FAKE, scores=FAKE, out=True)
    v.update(kw)
    # final_state and traj are not the summary's business
    o = NavTestOut(v["reached"], v["steps"], v["best"], None, None)
    with pytest.raises(NavError, match="invalid argument"):
        navlib.nav_pop_test_summary(C.byref(o) if v["out"] else None, v["n"], v["epm"],
                                    v["scores"], None)


def test_binding_declares_the_entry_points():
    from nav._lib import SIGNATURES, NavPopScore
    assert {"nav_pop_test_summary", "nav_td3_pop_state_bytes", "nav_td3_pop_state_build",
            "nav_td3_pop_exploit"} <= {s[0] for s in SIGNATURES}
    assert C.sizeof(NavPopScore) == 32
    assert [f[0] for f in NavPopScore._fields_] == ["reached", "steps_reached", "sum_best",
                                                    "max_best"]


# ---- pbt_select
def score(success, best):
    return {"success_rate": success, "mean_best_distance": best}


def obeys_the_entry_point(src, dst, P):
    assert len(src) == len(dst) and (P < 2 or 1 <= len(dst) <= P - 1)
    assert all(0 <= i < P for i in src + dst)
    assert len(set(dst)) == len(dst) and not set(dst) & set(src)


def test_select_quarter_of_eight():
    from nav import pbt_select
    #          0     1     2     3     4     5     6     7
    rates = [0.50, 0.90, 0.10, 0.70, 0.95, 0.20, 0.60, 0.30]
    sc = [score(r, 10.0) for r in rates]
    src, dst = pbt_select(sc, frac=0.25)
    assert (src, dst) == ([4, 1], [2, 5])  # worst first, the j-th worst from the j-th best
    obeys_the_entry_point(src, dst, 8)
    # the second key: the smaller mean best distance wins at equal success
    sc = [score(0.5, d) for d in (9.0, 3.0, 12.0, 7.0, 30.0, 8.0, 1.0, 20.0)]
    assert pbt_select(sc, frac=0.25) == ([6, 1], [4, 7])


def test_select_ties_go_to_the_lower_index():
    from nav import pbt_select
    sc = [score(0.5, 10.0) for _ in range(8)]
    assert pbt_select(sc, frac=0.25) == ([0, 1], [7, 6])
    sc[3] = score(0.9, 10.0)
    assert pbt_select(sc, frac=0.25) == ([3, 0], [7, 6])


def test_select_counts():
    from nav import pbt_select
    sc = [score(m / 8, 10.0) for m in range(8)]
    src, dst = pbt_select(sc, frac=0.9)  # capped at P // 2
    assert (src, dst) == ([7, 6, 5, 4], [0, 1, 2, 3])
    obeys_the_entry_point(src, dst, 8)
    assert pbt_select(sc, frac=0.01) == ([7], [0])  # at least one for P >= 2
    assert pbt_select(sc[:1], frac=0.25) == ([], [])
    assert pbt_select([], frac=0.25) == ([], [])
    assert pbt_select(sc[:2], frac=0.25) == ([1], [0])
    assert pbt_select(sc[:3], frac=0.9) == ([2], [0])
    for P_ in range(2, 12):
        for frac in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0):
            s, d = pbt_select(sc[:1] * P_, frac=frac, rng=np.random.default_rng(P_))
            obeys_the_entry_point(s, d, P_)
            assert len(d) == max(1, min(int(frac * P_), P_ // 2))


def test_select_with_a_generator_repeats():
    from nav import pbt_select
    sc = [score(m / 16, 10.0) for m in range(16)]
    a = pbt_select(sc, frac=0.5, rng=np.random.default_rng(11))
    b = pbt_select(sc, frac=0.5, rng=np.random.default_rng(11))
    assert a == b
    src, dst = a
    assert dst == list(range(8)) and set(src) <= set(range(8, 16))
    obeys_the_entry_point(src, dst, 16)


def test_select_custom_fitness_reverses():
    from nav import pbt_select
    sc = [score(m / 8, 10.0) for m in range(8)]
    src, dst = pbt_select(sc, frac=0.25, fitness=lambda s: -s["success_rate"])
    assert (src, dst) == ([0, 1], [7, 6])


# ---- the explore rule
class Picks:
    """rng.choice from a fixed list of picks."""

    def __init__(self, picks):
        self.picks = list(picks)

    def choice(self, options):
        v = self.picks.pop(0)
        assert v in options
        return v


def test_explore_rule():
    from nav.population import pbt_explore
    values = {"critic_lr": 1e-3, "gamma": 0.99, "max_action": 5.0, "demo_factor": 10.0}
    out = pbt_explore(values, {"critic_lr": (1e-5, 1e-2), "demo_factor": (1.0, 100.0)},
                      Picks([0.8, 1.25]))
    assert out == {"critic_lr": 1e-3 * 0.8, "demo_factor": 10.0 * 1.25}
    # clipped to the bounds, either side
    assert pbt_explore(values, {"gamma": (0.9, 0.999)}, Picks([1.25])) == {"gamma": 0.999}
    assert pbt_explore(values, {"max_action": (4.5, 5.0)}, Picks([0.8])) == {"max_action": 4.5}
    assert pbt_explore(values, {"max_action": (1.0, 1.0)}, Picks([1.25])) == {"max_action": 1.0}
    assert pbt_explore(values, None, Picks([])) == {}
    # a numpy generator draws one of the two factors
    g = np.random.default_rng(3)
    seen = {pbt_explore(values, {"critic_lr": (0.0, 1.0)}, g)["critic_lr"] for _ in range(32)}
    assert seen == {1e-3 * 0.8, 1e-3 * 1.25}


@pytest.mark.parametrize("key", ["bogus", "seed", "world_size", "init_region_size",
                                 "max_goal_draws", "policy_update_delay", "batch_size",
                                 "num_epochs", "net", "initial_noise", "path_length0",
                                 "path_increase", "seed_lo"])
def test_explore_refuses_unknown_and_shared_keys(key):
    from nav.population import PBT_EXPLORE_KEYS, pbt_explore
    assert key not in PBT_EXPLORE_KEYS
    with pytest.raises(KeyError, match="cannot be explored"):
        pbt_explore({key: 1.0}, {key: (0.0, 2.0)}, Picks([0.8]))


def test_explorable_keys_are_float_fields_of_the_structs():
    from nav import config as K
    from nav._lib import NavParams
    from nav.population import PBT_PARAM_KEYS, PBT_TD3_KEYS
    kinds = dict(NavParams._fields_)
    assert all(kinds[k] is C.c_double for k in PBT_PARAM_KEYS)
    import dataclasses
    declared = {f.name: f.type for f in dataclasses.fields(K.TD3Config)}
    assert all(declared[k] in (float, "float") for k in PBT_TD3_KEYS)
