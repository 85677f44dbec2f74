"""Population learner, host side: the argument validation of nav_td3_pop_table_build and the
*_pop launch entry points (every rejected condition returns NAV_EINVAL before any HIP call: no
kernel is launched by these calls, so no GPU is needed), nav_mlp_wgrad_splits_pop against
nav_mlp_wgrad_splits, and the trainer's keyword check."""
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
P, B, CAP, H, NH = 3, 100, 4096, 64, 3


@pytest.fixture(scope="module")
def navlib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib()


member = functools.partial(td3_member, hidden=H, n_hidden=NH, cap=CAP)


class Args:
    """A valid argument set of the entry points; a case alters one thing."""

    def __init__(self, **kw):
        from nav._lib import NavTd3Member
        self.m = [member(**kw) for _ in range(P)]
        self.n, self.B, self.table, self.size = P, B, FAKE, 3000
        self.sc, self.sa, self.group, self.splits = 1, 1, 0, 1
        self.soft, self.bc1, self.bc2s = 0, 0.1, 0.03
        self._T = NavTd3Member

    def arr(self):
        return (self._T * len(self.m))(*self.m)

    def calls(self, L):
        a = self.arr()
        return {
            "build": lambda: L.nav_td3_pop_table_build(a, self.n, self.B, self.sc, self.sa,
                                                       self.table, None),
            "critic": lambda: L.nav_td3_critic_rows_pop(a, self.n, self.B, self.table, self.size,
                                                        0, -1, None),
            "actor": lambda: L.nav_td3_actor_rows_pop(a, self.n, self.B, self.table, self.size,
                                                      0, None),
            "wgrad": lambda: L.nav_mlp_wgrad_pop(a, self.n, self.B, self.table, self.group,
                                                 self.splits, None),
            "reduce": lambda: L.nav_grad_reduce_adam_pop(a, self.n, self.B, self.table,
                                                         self.group, 0.9, 0.999, 1e-8, self.bc1,
                                                         self.bc2s, self.soft, None),
        }


ALL = ("build", "critic", "actor", "wgrad", "reduce")
ROWS = ("build", "critic", "actor")


def _capacity(a):
    a.m[2].replay.capacity = CAP // 2


# (what is wrong, the change, the entry points that must refuse it)
BAD = [
    ("no members", _set("n", 0), ALL),
    ("257 members", _set("n", 257), ALL),
    ("B = 0", _set("B", 0), ALL),
    ("no table", _set("table", None), ALL),
    ("another hidden width", _net_field("actor", "hidden", 32), ALL),
    ("another padded width", _net_field("target_actor", "hidden_pad", 96), ALL),
    ("another depth", _net_field("critics", "n_hidden", 2, 1), ALL),
    ("another target depth", _net_field("target_critics", "n_hidden", 2, 0, m=2), ALL),
    ("another critic input", _net_field("critics", "d_in", 3, 0, m=0), ALL),
    ("another ring capacity", _capacity, ALL),
    ("size = 0", _set("size", 0), ("critic", "actor")),
    ("size > capacity", _set("size", CAP + 1), ("critic", "actor")),
    ("no ring rows", lambda a: setattr(a.m[1].replay, "rows", None), ROWS),
    ("no actor params", _net_field("actor", "params", None), ALL),
    ("no target critic image", _net_field("target_critics", "packed", None, 1), ROWS),
    ("no critic batch", _member_field("batch", None), ALL),
    ("no actor batch", _member_field("batch_actor", None), ALL),
    ("no dq", _member_field("dq", None, 1), ALL),
    ("no loss_part", _member_field("loss_part", None, 0), ROWS),
    ("no critic masks", _member_field("masks", None, 1), ALL),
    ("no actor masks", _member_field("masks_actor", None), ALL),
    ("no da", _member_field("da", None), ALL),
    ("no critic edge slabs", _member_field("edge_slabs", None, 0), ALL),
    ("no actor edge slabs", _member_field("edge_slabs_actor", None), ALL),
    # 3 hidden layers: the middle layer's rows are saved (save_mask / dz_save_mask = 2)
    ("save_mask without acts", _member_field("acts", None, 0), ALL),
    ("dz_save_mask without dz", _member_field("dz", None, 1), ALL),
    ("actor save_mask without acts", _member_field("acts_actor", None), ALL),
    ("actor dz_save_mask without dz", _member_field("dz_actor", None), ALL),
    ("no hidden slabs", _member_field("hidden_slabs", None, 1), ("build", "wgrad", "reduce")),
    ("no moments", _member_field("v_critic", None, 0), ("build", "wgrad", "reduce")),
    ("no actor moments", _member_field("m_actor", None), ("build", "wgrad", "reduce")),
    ("splits_critic = 0", _set("sc", 0), ("build",)),
    ("splits_actor = 0", _set("sa", 0), ("build",)),
    ("splits = 0", _set("splits", 0), ("wgrad",)),
    ("group = 2", _set("group", 2), ("wgrad", "reduce")),
    ("soft update on the critics", _set("soft", 1), ("reduce",)),
    ("bc1 = 0", _set("bc1", 0.0), ("reduce",)),
]


@pytest.mark.parametrize("what,change,entries", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_on_the_host(navlib, what, change, entries):
    from nav._lib import NavError
    a = Args()
    change(a)
    calls = a.calls(navlib)
    for e in entries:
        with pytest.raises(NavError, match="invalid argument"):
            calls[e]()


def test_table_bytes(navlib):
    from nav._lib import NavError
    one = navlib.nav_td3_pop_table_bytes(1)
    assert one > 0 and one % 8 == 0
    assert navlib.nav_td3_pop_table_bytes(256) == 256 * one
    for bad in (0, -1, 257):
        with pytest.raises(NavError):
            navlib.nav_td3_pop_table_bytes(bad)


SHAPES = [(n_nets, d_out, hp, nh, M)
          for n_nets, d_out in ((2, 1), (1, 2))
          for hp, nh in ((224, 3), (256, 2), (128, 2), (64, 2), (32, 1))
          for M in (0, 100, 2112, 4096, 32768, 1 << 20)]


def test_wgrad_splits_pop(navlib):
    from nav._lib import NavError
    for n_nets, d_out, hp, nh, M in SHAPES:
        lone = navlib.nav_mlp_wgrad_splits(n_nets, d_out, hp, nh, M)
        assert navlib.nav_mlp_wgrad_splits_pop(1, n_nets, d_out, hp, nh, M) == lone
        last = lone
        for members in (2, 3, 8, 64, 256):
            s = navlib.nav_mlp_wgrad_splits_pop(members, n_nets, d_out, hp, nh, M)
            assert 1 <= s <= last, (members, n_nets, d_out, hp, nh, M)
            last = s
    # the chip's 256 tile workgroups over 8 members' twins: 8 jobs of 256 x 32 per critic
    assert navlib.nav_mlp_wgrad_splits_pop(8, 2, 1, 256, 2, 4096) == 2
    assert navlib.nav_mlp_wgrad_splits(2, 1, 256, 2, 4096) == 8
    for bad in ((0, 2, 1, 256, 2, 64), (257, 2, 1, 256, 2, 64), (2, 3, 1, 256, 2, 64),
                (2, 2, 1, 200, 2, 64), (2, 2, 1, 256, 0, 64)):
        with pytest.raises(NavError):
            navlib.nav_mlp_wgrad_splits_pop(*bad)


def test_binding_declares_the_entry_points():
    from nav._lib import SIGNATURES
    assert {"nav_td3_pop_table_bytes", "nav_td3_pop_table_build", "nav_td3_critic_rows_pop",
            "nav_td3_actor_rows_pop", "nav_mlp_wgrad_splits_pop", "nav_mlp_wgrad_pop",
            "nav_grad_reduce_adam_pop"} <= {s[0] for s in SIGNATURES}


def test_trainer_keywords():
    from nav.population import PopulationTrainer
    with pytest.raises(ValueError, match="streams"):
        PopulationTrainer([{}, {}], learner="batched", streams=2)
    with pytest.raises(ValueError, match="learner"):
        PopulationTrainer([{}], learner="fused")
