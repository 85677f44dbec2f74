"""Population training, host side: sweep_grid's cross product, the routing of member overrides,
and the host-side argument validation of nav_pop_table_build / nav_act_tick_pop /
nav_test_rollout_pop: every rejected condition returns NAV_EINVAL before any HIP call (no kernel
is launched by these calls, so no GPU is needed)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "nav", "libnavenv.so")
FAKE = 16  # a non-null pointer value that is never dereferenced on the host
P, EPM, CAP = 3, 128, 384


@pytest.fixture(scope="module")
def navlib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib()


def test_sweep_grid_cross_product():
    from nav.population import sweep_grid
    assert sweep_grid() == [{}]
    assert sweep_grid(demo_factor=[10, 30, 50, 70]) == [{"demo_factor": v}
                                                        for v in (10, 30, 50, 70)]
    g = sweep_grid(initial_noise=[1.0, 0.5], noise_decay=[0.5, 0.75, 0.9], seed=[1, 2])
    assert len(g) == 12
    # the last axis varies fastest, every combination once
    assert g[0] == {"initial_noise": 1.0, "noise_decay": 0.5, "seed": 1}
    assert g[1] == {"initial_noise": 1.0, "noise_decay": 0.5, "seed": 2}
    assert g[2] == {"initial_noise": 1.0, "noise_decay": 0.75, "seed": 1}
    assert g[-1] == {"initial_noise": 0.5, "noise_decay": 0.9, "seed": 2}
    assert len({tuple(sorted(m.items())) for m in g}) == 12


def test_override_routing():
    from nav.population import route_overrides
    params, cfg, extra = route_overrides({"demo_factor": 30.0, "path_length0": 6,
                                          "critic_lr": 1e-4, "tau": 0.01, "max_action": 4.0,
                                          "initial_noise": 0.5, "seed": 7})
    assert params == {"demo_factor": 30.0, "path_length0": 6, "max_action": 4.0}
    assert cfg == {"critic_lr": 1e-4, "tau": 0.01, "max_action": 4.0}
    assert extra == {"initial_noise": 0.5, "seed": 7}
    assert route_overrides({}) == ({}, {}, {})
    for bad in ("demo_faktor", "batch_size", "net", "hidden"):
        with pytest.raises(KeyError, match=bad):
            route_overrides({"noise_decay": 0.5, bad: 1})


def test_binding_declares_the_entry_points():
    from nav._lib import SIGNATURES
    assert {"nav_pop_table_bytes", "nav_pop_table_build", "nav_act_tick_pop",
            "nav_test_rollout_pop"} <= {s[0] for s in SIGNATURES}


class Args:
    """A valid argument set of the three entry points on fake pointers; a case alters one thing."""

    def __init__(self):
        from nav._lib import (NavEnvSoa, NavMlp, NavParams, NavReplay, NavStepOut, NavTestOut,
                              params_struct)
        self.params = (NavParams * P)(*[params_struct(demo_factor=10.0 * (m + 1))
                                        for m in range(P)])
        self.actors = (NavMlp * P)(*[NavMlp(2, 2, 64, 64, 2, FAKE, FAKE) for _ in range(P)])
        self.replays = (NavReplay * P)(*[NavReplay(FAKE, CAP) for _ in range(P)])
        self.n_members, self.epm, self.table = P, EPM, FAKE
        self.env = NavEnvSoa(P * EPM, *([FAKE] * 9))
        self.out = NavStepOut(FAKE, FAKE, FAKE, FAKE)
        self.test_out = NavTestOut(FAKE, FAKE, FAKE, FAKE, None)
        self.field = FAKE
        self.demo_xy = self.demo_off = self.cell_start = self.cand = None
        self.epg = 64

    def build(self, L):
        return L.nav_pop_table_build(self.params, self.actors, self.replays, self.n_members,
                                     self.epm, self.table, None)

    def tick(self, L):
        return L.nav_act_tick_pop(self.params, self.actors, self.replays, self.n_members,
                                  self.epm, self.table, C.byref(self.env), self.field, None, 0, 0,
                                  0, C.byref(self.out), self.demo_xy, self.demo_off, self.epg,
                                  self.cell_start, self.cand, None, None, None)

    def test(self, L):
        return L.nav_test_rollout_pop(self.params, self.actors, self.n_members, self.epm,
                                      self.table, C.byref(self.env), self.field, None, 0, 12,
                                      C.byref(self.test_out), None)


def _epm_not_64(a):
    a.epm = 96
    a.env.n = P * 96


def _epm_not_epg(a):  # only where a demo set is given: the tick
    a.demo_xy, a.cell_start, a.cand, a.epg = FAKE, FAKE, FAKE, 48


def _set(field, m, value):
    def f(a):
        setattr(a.actors[m], field, value)
    return f


def _setp(field, m, value):
    def f(a):
        setattr(a.params[m], field, value)
    return f


def _cap_differs(a):
    a.replays[2].capacity = CAP + 64


def _cap_small(a):
    for m in range(P):
        a.replays[m].capacity = 64


def _null(name):
    def f(a):
        setattr(a, name, None)
    return f


def _null_ring_rows(a):
    a.replays[1].rows = None


def _null_actor_params(a):
    a.actors[2].params = None


def _n_mismatch(a):
    a.env.n = P * EPM + 64


def _n_members(n):  # (the env count follows, so that the member count alone is at fault)
    def f(a):
        a.n_members, a.env.n = n, n * EPM
    return f


# (case, alteration, entry points it applies to)
ALL, TICK, RINGS = ("build", "tick", "test"), ("tick",), ("build", "tick")
CASES = [
    ("no members", _n_members(0), ALL),
    ("257 members", _n_members(257), ALL),
    ("envs_per_member not a multiple of 64", _epm_not_64, ALL),
    ("envs_per_member not a multiple of envs_per_group", _epm_not_epg, TICK),
    ("d_in differs", _set("d_in", 1, 4), ALL),
    ("d_out differs", _set("d_out", 1, 1), ALL),
    ("hidden differs", _set("hidden", 2, 60), ALL),
    ("hidden_pad differs", _set("hidden_pad", 1, 96), ALL),
    ("n_hidden differs", _set("n_hidden", 2, 3), ALL),
    ("world_size differs", _setp("world_size", 1, 50.0), ALL),
    ("init_region_size differs", _setp("init_region_size", 2, 20.0), ALL),
    ("seed_lo differs", _setp("seed_lo", 1, 5), ALL),
    ("seed_hi differs", _setp("seed_hi", 2, 5), ALL),
    ("max_goal_draws differs", _setp("max_goal_draws", 1, 100), ALL),
    ("ring capacities differ", _cap_differs, RINGS),
    ("ring capacity below envs_per_member", _cap_small, RINGS),
    ("null params", _null("params"), ALL),
    ("null actors", _null("actors"), ALL),
    ("null table", _null("table"), ALL),
    ("null replays", _null("replays"), TICK),
    ("null ring rows", _null_ring_rows, RINGS),
    ("null actor parameters", _null_actor_params, ALL),
    ("null field", _null("field"), ("tick", "test")),
    ("env.n is not n_members * envs_per_member", _n_mismatch, ("tick", "test")),
]


@pytest.mark.parametrize("what,alter,entries", CASES, ids=[c[0] for c in CASES])
def test_rejected_before_any_hip_call(navlib, what, alter, entries):
    from nav._lib import NavError
    for entry in entries:
        a = Args()
        alter(a)
        with pytest.raises(NavError, match="invalid argument"):
            getattr(a, entry)(navlib)


def test_table_bytes(navlib):
    from nav._lib import NavError
    one = navlib.nav_pop_table_bytes(1)
    assert one > 0 and navlib.nav_pop_table_bytes(P) == P * one
    for bad in (0, -1, 257):
        with pytest.raises(NavError, match="invalid argument"):
            navlib.nav_pop_table_bytes(bad)
