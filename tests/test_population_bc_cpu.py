"""Populations that learn from demonstrations, host side: the argument validation of
nav_td3_pop_bc_table_build, nav_td3_mix_idx_pop and nav_td3_actor_rows_bc_pop (every rejected
condition returns NAV_EINVAL before any HIP call: no kernel is launched by these calls, so no GPU
is needed; an accepted call would launch, so every case here has to be refused), the BC table's
size, the group-to-member bookkeeping of the members' demonstration tails, and what `explore` may
perturb."""
import ctypes as C
import functools
import os
import subprocess

import pytest

from abi_args import member_field as _member_field
from abi_args import net_field as _net_field
from abi_args import set_attr as _set
from abi_args import td3_member
from conftest import PKG

LIB = os.path.join(PKG, "nav", "libnavenv.so")
FAKE = 16  # a non-null pointer value that is never dereferenced on the host
IDX_C, IDX_A = 4096, 8192  # the members' (fake) index arrays
P, B, CAP, H, NH = 3, 100, 4096, 64, 3
NEW = ("nav_td3_pop_bc_table_bytes", "nav_td3_pop_bc_table_build", "nav_td3_mix_idx_pop",
       "nav_td3_actor_rows_bc_pop")


@pytest.fixture(scope="module")
def navlib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib()


member = functools.partial(td3_member, hidden=H, n_hidden=NH, cap=CAP, idx=(IDX_C, IDX_A))


def member_bc(b_demo=7, n_demo=37, q=1.0, bc=0.5):
    from nav._lib import NavTd3MemberBc
    return NavTd3MemberBc(b_demo, n_demo, q, bc, IDX_C, IDX_A, FAKE)


class Args:
    """A valid argument set of the three entry points; a case alters one thing."""

    def __init__(self):
        self.m = [member() for _ in range(P)]
        self.bc = [member_bc(0, 0, 1.0, 0.0), member_bc(), member_bc(B, 1, 0.25, 3.0)]
        self.n, self.B, self.table, self.size, self.no_bc = P, B, FAKE, 3000, False

    def calls(self, L):
        from nav._lib import NavTd3Member, NavTd3MemberBc
        a = (NavTd3Member * len(self.m))(*self.m)
        b = None if self.no_bc else (NavTd3MemberBc * len(self.bc))(*self.bc)
        raw = L.raw
        return {
            "build": lambda: raw.nav_td3_pop_bc_table_build(a, b, self.n, self.B, self.table,
                                                            None),
            "mix": lambda: raw.nav_td3_mix_idx_pop(a, b, self.n, self.B, self.table, self.size,
                                                   0, 1, None),
            "actor": lambda: raw.nav_td3_actor_rows_bc_pop(a, b, self.n, self.B, self.table,
                                                           self.size, 0, None),
        }


ALL = ("build", "mix", "actor")
LAUNCH = ("mix", "actor")


def _bc_field(name, value, m=1):
    def f(a):
        setattr(a.bc[m], name, value)
    return f


def _both(*fs):
    def f(a):
        for g in fs:
            g(a)
    return f


# (what is wrong, the change, the entry points that must refuse it)
BAD = [
    # what nav_td3_actor_rows_pop checks
    ("no members", _set("n", 0), ALL),
    ("257 members", _set("n", 257), ALL),
    ("B = 0", _set("B", 0), ALL),
    ("another hidden width", _net_field("actor", "hidden", 32), ALL),
    ("another depth", _net_field("critics", "n_hidden", 2, 1), ALL),
    ("another critic input", _net_field("critics", "d_in", 3, 0, m=0), ALL),
    ("another ring capacity", lambda a: setattr(a.m[2].replay, "capacity", CAP // 2), ALL),
    ("size = 0", _set("size", 0), LAUNCH),
    ("size > capacity", _set("size", CAP + 1), LAUNCH),
    ("no ring rows", lambda a: setattr(a.m[1].replay, "rows", None), ALL),
    ("no actor params", _net_field("actor", "params", None), ALL),
    ("no actor batch", _member_field("batch_actor", None), ALL),
    ("no da", _member_field("da", None), ALL),
    ("no actor masks", _member_field("masks_actor", None), ALL),
    ("no actor edge slabs", _member_field("edge_slabs_actor", None), ALL),
    ("actor save_mask without acts", _member_field("acts_actor", None), ALL),
    ("actor dz_save_mask without dz", _member_field("dz_actor", None), ALL),
    # the issue's list
    ("no bc array", _set("no_bc", True), ALL),
    ("no table", _set("table", None), ALL),
    ("B_demo < 0", _bc_field("B_demo", -1), ALL),
    ("B_demo > B", _bc_field("B_demo", B + 1), ALL),
    ("bc_weight on no rows", _bc_field("bc_weight", 0.5, m=0), ALL),
    ("demonstration rows without a tail", _bc_field("n_demo", 0), ALL),
    ("a negative tail", _bc_field("n_demo", -3, m=2), ALL),
    ("no bc_part", _bc_field("bc_part", None, m=0), ALL),
    ("no idx_critic", _both(_bc_field("idx_critic", None), _member_field("idx_critic", None)),
     ALL),
    ("no idx_actor", _both(_bc_field("idx_actor", None, m=2),
                           _member_field("idx_actor", None, m=2)), ALL),
    ("idx_critic is not the member's", _bc_field("idx_critic", IDX_C + 8), ALL),
    ("idx_actor is not the member's", _member_field("idx_actor", IDX_C, m=0), ALL),
    ("the member injects no idx_actor", _member_field("idx_actor", None), ALL),
]


@pytest.mark.parametrize("what,change,entries", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_on_the_host(navlib, what, change, entries):
    from nav._lib import NAV_EINVAL
    a = Args()
    change(a)
    calls = a.calls(navlib)
    for e in entries:
        assert calls[e]() == NAV_EINVAL, e


def test_binding_declares_and_the_library_exports_the_entry_points(navlib):
    from nav._lib import SIGNATURES
    assert set(NEW) <= {s[0] for s in SIGNATURES}
    for name in NEW:
        assert getattr(navlib.raw, name) is not None
    assert navlib.nav_abi_version() == 11


def test_bc_table_bytes(navlib):
    from nav._lib import NavError
    one = navlib.nav_td3_pop_bc_table_bytes(1)
    assert one > 0 and one % 8 == 0
    for n in range(1, 257):
        assert navlib.nav_td3_pop_bc_table_bytes(n) == n * one
    for bad in (0, 257):
        with pytest.raises(NavError):
            navlib.nav_td3_pop_bc_table_bytes(bad)


def test_member_bc_struct_layout():
    """nav_td3_member_bc as include/navenv.h declares it: two int64, two floats, three pointers."""
    from nav._lib import NavTd3MemberBc
    assert C.sizeof(NavTd3MemberBc) == 48
    assert [NavTd3MemberBc.B_demo.offset, NavTd3MemberBc.n_demo.offset,
            NavTd3MemberBc.q_weight.offset, NavTd3MemberBc.bc_weight.offset,
            NavTd3MemberBc.idx_critic.offset, NavTd3MemberBc.idx_actor.offset,
            NavTd3MemberBc.bc_part.offset] == [0, 8, 16, 20, 24, 32, 40]


def test_member_demo_groups():
    from nav.population import member_demo_groups
    groups, demos = member_demo_groups(1, 256, 128)
    assert list(groups) == [2, 3] and list(demos) == list(range(6, 12))
    groups, demos = member_demo_groups(0, 256, 128)
    assert list(groups) == [0, 1] and list(demos) == list(range(0, 6))
    # one group per member, and another demonstration count
    assert [list(r) for r in member_demo_groups(2, 128, 128)] == [[2], [6, 7, 8]]
    assert [list(r) for r in member_demo_groups(1, 128, 64, n_demos=2)] == [[2, 3], [4, 5, 6, 7]]
    # the members' demonstrations partition the CEM's list
    seen = [d for m in range(4) for d in member_demo_groups(m, 512, 128)[1]]
    assert seen == list(range(4 * 4 * 3))
    with pytest.raises(ValueError, match="whole env groups"):
        member_demo_groups(1, 256, 96)
    with pytest.raises(ValueError, match="whole env groups"):
        member_demo_groups(0, 128, 256)


class Picks:
    """rng.choice's stand-in: the factors in the given order."""

    def __init__(self, factors):
        self.factors = list(factors)

    def choice(self, _):
        return self.factors.pop(0)


def test_weights_can_be_explored_and_demo_fraction_cannot():
    from nav.population import PBT_EXPLORE_KEYS, PBT_TD3_KEYS, pbt_explore
    assert {"bc_weight", "q_weight"} <= PBT_TD3_KEYS and "demo_fraction" not in PBT_EXPLORE_KEYS
    values = {"bc_weight": 1.0, "q_weight": 0.5, "demo_fraction": 0.25}
    out = pbt_explore(values, {"bc_weight": (0.0, 4.0), "q_weight": (0.0, 0.6)},
                      Picks([0.8, 1.25]))
    assert out == {"bc_weight": 0.8, "q_weight": 0.6}
    with pytest.raises(KeyError, match="cannot be explored"):
        pbt_explore(values, {"demo_fraction": (0.0, 1.0)}, Picks([0.8]))


def test_overrides_route_the_three_keys_to_the_learner():
    from nav.population import BC_KEYS, route_overrides
    params, cfg, extra = route_overrides({"demo_fraction": 0.25, "bc_weight": 1.0,
                                          "q_weight": 0.5, "demo_factor": 30.0})
    assert set(cfg) == set(BC_KEYS) and params == {"demo_factor": 30.0} and extra == {}


def test_trainer_refuses_the_keys_without_demonstrations_or_whole_groups():
    """Both before anything touches the device."""
    from nav.population import PopulationTrainer
    for key in ("demo_fraction", "bc_weight", "q_weight"):
        with pytest.raises(ValueError, match="demos=True"):
            PopulationTrainer([{}, {key: 0.5}], demos=False)
    with pytest.raises(ValueError, match="whole env groups"):
        PopulationTrainer([{"demo_fraction": 0.25, "bc_weight": 1.0}], envs_per_member=256,
                          envs_per_group=96)


def test_replay_ring_takes_a_tailed_slice_of_a_population_tensor():
    import torch
    from nav.vec_env import ReplayRing
    pool = torch.zeros(2, 8 + 3, 8)
    ring = ReplayRing(8, "cpu", rows=pool[1], tail=3)
    assert ring.rows.shape == (8, 8) and ring.tail.shape == (3, 8)
    assert ring.rows.data_ptr() == pool[1].data_ptr() == ring.desc().rows
    assert ring.tail.data_ptr() == pool[1].data_ptr() + 8 * 8 * 4 and ring.desc().capacity == 8
    assert ring.rows.is_contiguous() and ring.tail.is_contiguous()
    with pytest.raises(AssertionError):
        ReplayRing(8, "cpu", rows=pool[1])  # a tailed slice given as a plain ring


def test_fp32_chain_of_the_fp64_member_stays_inside_the_band_cap(orc):
    """A condition of the GPU test's fp64 comparison (tests/test_gpu_population_bc.py), as
    tests/test_bc_cpu.py establishes it for the single-member cases: on the rows the mix draws for
    the judged member, the fp32 chain's own ReLU decisions stay inside mlp_ref's band cap, for the
    actor and for the critic on (s, pi(s))."""
    import torch

    import mlp_ref as R
    import pop_bc_ref as PB
    f = PB.FP64
    case, storage = PB.fp64_member_rows()
    idx = PB.host_mix_idx(orc, PB.member_seed(f["member"]), f["B"], f["b_demo"], PB.FILL, PB.CAP,
                          PB.N_TAIL, PB.COUNTER, actor=True)
    assert all(i >= PB.CAP for i in idx[:f["b_demo"]]) and max(idx[f["b_demo"]:]) < PB.FILL
    rows = storage[torch.tensor(idx)]
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    s = rows[:, :2]
    a64, zs_a, _ = R.mlp_forward(la, s)
    a32, zs_a32, _ = R.mlp_forward(la, s, torch.float32)
    inside, entries = R.relu_band(la, s, zs_a, [z > 0 for z in zs_a32])
    x = torch.cat([s.double(), a64], 1)
    _, zs_c, _ = R.mlp_forward(lc, x)
    _, zs_c32, _ = R.mlp_forward(lc, torch.cat([s, a32], 1), torch.float32)
    bar_a = R.bar("a", R.rel_err(a32, a64)) * float(a64.abs().max())
    extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ lc[0][0][:, 2:4].double().abs().t()
    i2, e2 = R.relu_band(lc, x, zs_c, [z > 0 for z in zs_c32], extra0=extra)
    R.assert_band_cap(inside + i2, entries + e2)


def test_sweep_accepts_the_new_axes_and_bounds():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(PKG), "tools"))
    import sweep
    assert sweep.parse_axis("bc_weight=0,0.5,1") == ("bc_weight", [0, 0.5, 1])
    assert sweep.parse_explore("bc_weight=0:4") == ("bc_weight", (0.0, 4.0))
    members, _ = sweep.members_of({"bc_weight": [0, 0.5, 1], "demo_fraction": [0.25]}, 1, 0)
    assert members == [{"bc_weight": w, "demo_fraction": 0.25} for w in (0, 0.5, 1)]
