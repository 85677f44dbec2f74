"""The plain learner entry points, host side: every argument set below is refused with the raw
status NAV_EINVAL before any HIP call (no kernel is launched, the dummy pointers are never
followed, so no GPU is needed), and nav_mlp_wgrad_splits / nav_mlp_wgrad_splits_pop return the
split counts recorded from the library before the learner sources were split into wgrad.h,
reduce_adam.h, learner_host.h, learner_kernels.hip and learner_pop.hip. The population entry
points' table is tests/test_population_learner_cpu.py."""
import ctypes as C

import pytest

from abi_args import EINVAL, F, Call, load_raw
from abi_args import v as _v

NAN = float("nan")


@pytest.fixture(scope="module")
def raw():
    return load_raw()


def net(d_in=4, d_out=1, hidden=64, n_hidden=2):
    from nav._lib import NavMlp
    return NavMlp(d_in, d_out, hidden, hidden, n_hidden, F, F)


def nets(*ns):
    from nav._lib import NavMlp
    return (NavMlp * len(ns))(*ns)


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def floats(*v):
    return (C.c_float * len(v))(*v)


TWINS = lambda: nets(net(), net())  # noqa: E731
PAIR = lambda: ptrs(F, F)  # noqa: E731
_ADAM = dict(beta1=_v(0.9), beta2=_v(0.999), eps=_v(1e-8), step_size=lambda: floats(1e-3, 1e-3),
             bc2_sqrt=lambda: floats(0.5, 0.5))
_POLY = dict(net_targets=TWINS, targets=lambda: nets(net()), sources=lambda: nets(net()),
             n_pairs=_v(1), tau=_v(0.005))
_REDUCE = dict(nets=TWINS, n_nets=_v(2), hidden_slabs=PAIR, splits=_v(1), edge_slabs=PAIR,
               edge_blocks=_v(4), grads=PAIR)
_MOMENTS = dict(m=PAIR, v=PAIR)
_ADAM_MULTI = dict(nets=TWINS, n_nets=_v(2), grads=PAIR, **_MOMENTS, **_ADAM, grad_div=_v(1.0))

CALLS = {c.fn: c for c in (
    Call("nav_grad_reduce", net=lambda: C.byref(net(n_hidden=1)), hidden_slabs=_v(F),
         splits=_v(1), edge_slabs=_v(F), edge_blocks=_v(4), grad=_v(F), stream=_v(None)),
    Call("nav_grad_reduce_multi", **_REDUCE, stream=_v(None)),
    Call("nav_grad_reduce_adam", **_REDUCE, **_MOMENTS, **_ADAM, stream=_v(None)),
    Call("nav_grad_reduce_adam_polyak", **_REDUCE, **_MOMENTS, **_ADAM, **_POLY,
         stream=_v(None)),
    Call("nav_adam_multi", **_ADAM_MULTI, stream=_v(None)),
    Call("nav_adam_polyak_multi", **_ADAM_MULTI, **_POLY, stream=_v(None)),
    Call("nav_polyak_multi", targets=TWINS, sources=TWINS, n=_v(2), tau=_v(0.005),
         stream=_v(None)),
    Call("nav_polyak", target=lambda: C.byref(net()), source=lambda: C.byref(net()),
         tau=_v(0.005), stream=_v(None)),
    Call("nav_adam", net=lambda: C.byref(net()), grad=_v(F), m=_v(F), v=_v(F), beta1=_v(0.9),
         beta2=_v(0.999), eps=_v(1e-8), step_size=_v(1e-3), bc2_sqrt=_v(0.5), stream=_v(None)),
    Call("nav_mlp_wgrad", nets=TWINS, n_nets=_v(2), M=_v(64), inp=_v(F), ld_in=_v(8),
         in_col=_v(0), acts=_v(None), dz=_v(None), dy=PAIR, ld_dy=_v(1), masks=PAIR, slabs=PAIR,
         splits=_v(4), stream=_v(None)),
    Call("nav_mlp_wgrad_splits", n_nets=_v(2), d_out=_v(1), hidden_pad=_v(256), n_hidden=_v(2),
         M=_v(4096)),
)}

DEEP = lambda: C.byref(net(n_hidden=2))  # noqa: E731
BOTH_ADAM = ("nav_adam_multi", "nav_adam_polyak_multi")

# (entry point, what is wrong, the altered arguments)
BAD = [
    ("nav_grad_reduce", "no grad", dict(grad=_v(None))),
    ("nav_grad_reduce", "no edge slabs", dict(edge_slabs=_v(None))),
    ("nav_grad_reduce", "edge_blocks = 0", dict(edge_blocks=_v(0))),
    ("nav_grad_reduce", "splits = -1", dict(splits=_v(-1))),
    ("nav_grad_reduce", "2 hidden layers, no hidden slabs", dict(net=DEEP, hidden_slabs=_v(None))),
    ("nav_grad_reduce", "2 hidden layers, splits = 0", dict(net=DEEP, splits=_v(0))),
    ("nav_grad_reduce_multi", "n_nets = 0", dict(n_nets=_v(0))),
    ("nav_grad_reduce_multi", "n_nets = 3", dict(n_nets=_v(3))),
    ("nav_grad_reduce_multi", "another hidden_pad",
     dict(nets=lambda: nets(net(), net(hidden=128)))),
    ("nav_grad_reduce_multi", "another n_hidden", dict(nets=lambda: nets(net(), net(n_hidden=3)))),
    ("nav_grad_reduce_multi", "grads[1] NULL", dict(grads=lambda: ptrs(F, None))),
    ("nav_grad_reduce_multi", "edge_slabs[1] NULL", dict(edge_slabs=lambda: ptrs(F, None))),
    ("nav_grad_reduce_adam", "no m", dict(m=_v(None))),
    ("nav_grad_reduce_adam", "no v", dict(v=_v(None))),
    ("nav_grad_reduce_adam", "no step_size", dict(step_size=_v(None))),
    ("nav_grad_reduce_adam", "m[1] NULL", dict(m=lambda: ptrs(F, None))),
    ("nav_grad_reduce_adam_polyak", "no net_targets", dict(net_targets=_v(None))),
    ("nav_grad_reduce_adam_polyak", "n_pairs = 5", dict(n_pairs=_v(5))),
    ("nav_grad_reduce_adam_polyak", "n_pairs = -1", dict(n_pairs=_v(-1))),
    ("nav_grad_reduce_adam_polyak", "n_pairs = 1, no targets", dict(targets=_v(None))),
    ("nav_grad_reduce_adam_polyak", "a net target of another hidden_pad",
     dict(net_targets=lambda: nets(net(), net(hidden=128)))),
    ("nav_grad_reduce_adam_polyak", "a pair of another n_hidden",
     dict(sources=lambda: nets(net(n_hidden=3)))),
] + [case for fn in BOTH_ADAM for case in (
    (fn, "grad_div = 0", dict(grad_div=_v(0.0))),
    (fn, "grad_div < 0", dict(grad_div=_v(-2.0))),
    (fn, "grad_div NaN", dict(grad_div=_v(NAN))),
    (fn, "no bc2_sqrt", dict(bc2_sqrt=_v(None))),
    (fn, "n_nets = 3", dict(n_nets=_v(3))),
)] + [
    ("nav_adam_polyak_multi", "no net_targets", dict(net_targets=_v(None))),
    ("nav_adam_polyak_multi", "a pair of another parameter count",
     dict(sources=lambda: nets(net(d_in=2)))),
    ("nav_polyak_multi", "n = 0", dict(n=_v(0))),
    ("nav_polyak_multi", "n = 5", dict(n=_v(5))),
    ("nav_polyak_multi", "a pair of another hidden_pad",
     dict(sources=lambda: nets(net(), net(hidden=128)))),
    ("nav_polyak", "another n_hidden", dict(source=lambda: C.byref(net(n_hidden=3)))),
    ("nav_adam", "no grad", dict(grad=_v(None))),
    ("nav_adam", "no m", dict(m=_v(None))),
    ("nav_adam", "no v", dict(v=_v(None))),
    ("nav_mlp_wgrad", "n_nets = 3", dict(n_nets=_v(3))),
    ("nav_mlp_wgrad", "M = 0", dict(M=_v(0))),
    ("nav_mlp_wgrad", "splits = 0", dict(splits=_v(0))),
    ("nav_mlp_wgrad", "in_col + d_in > ld_in", dict(in_col=_v(5))),
    ("nav_mlp_wgrad", "3 hidden layers, no acts",
     dict(nets=lambda: nets(net(n_hidden=3), net(n_hidden=3)), dz=PAIR)),
    ("nav_mlp_wgrad", "another d_out", dict(nets=lambda: nets(net(), net(d_out=2)))),
    ("nav_mlp_wgrad", "slabs[1] NULL", dict(slabs=lambda: ptrs(F, None))),
    # 2 nets x 8 tile jobs (256 x 32 tiles at hidden_pad 256) x 2^27 splits = 2^31 workgroups
    ("nav_mlp_wgrad", "grid over 2^30 workgroups",
     dict(nets=lambda: nets(net(hidden=256), net(hidden=256)), splits=_v(1 << 27))),
    ("nav_mlp_wgrad_splits", "hidden_pad = 48", dict(hidden_pad=_v(48))),
    ("nav_mlp_wgrad_splits", "hidden_pad = 288", dict(hidden_pad=_v(288))),
    ("nav_mlp_wgrad_splits", "d_out = 3", dict(d_out=_v(3))),
    ("nav_mlp_wgrad_splits", "n_nets = 0", dict(n_nets=_v(0))),
    ("nav_mlp_wgrad_splits", "M = -1", dict(M=_v(-1))),
]


@pytest.mark.parametrize("fn,what,changed", BAD, ids=[f"{b[0]}-{b[1]}" for b in BAD])
def test_bad_arguments_return_einval(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == EINVAL


def test_every_listed_entry_point_has_a_case():
    assert {b[0] for b in BAD} == set(CALLS)


# nav_mlp_wgrad_splits at M = 0, 100, 32 768 and nav_mlp_wgrad_splits_pop at the same M for 1, 3
# and 16 members, keyed (n_nets, d_out, hidden_pad, n_hidden): what the library returned before the
# split of the learner sources
SPLIT_M = (0, 100, 32768)
SPLIT_MEMBERS = (1, 3, 16)
SPLITS = {
    (1, 1, 64, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 1, 64, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 64), (1, 1, 16))),
    (1, 1, 64, 3): ((1, 1, 64), ((1, 1, 64), (1, 1, 42), (1, 1, 8))),
    (1, 1, 128, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 1, 128, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 42), (1, 1, 8))),
    (1, 1, 128, 3): ((1, 1, 32), ((1, 1, 32), (1, 1, 10), (1, 1, 2))),
    (1, 1, 192, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 1, 192, 2): ((1, 1, 28), ((1, 1, 28), (1, 1, 9), (1, 1, 1))),
    (1, 1, 192, 3): ((1, 1, 14), ((1, 1, 14), (1, 1, 4), (1, 1, 1))),
    (1, 1, 256, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 1, 256, 2): ((1, 1, 32), ((1, 1, 32), (1, 1, 10), (1, 1, 2))),
    (1, 1, 256, 3): ((1, 1, 8), ((1, 1, 8), (1, 1, 2), (1, 1, 1))),
    (1, 2, 64, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 2, 64, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 64), (1, 1, 16))),
    (1, 2, 64, 3): ((1, 1, 64), ((1, 1, 64), (1, 1, 42), (1, 1, 8))),
    (1, 2, 128, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 2, 128, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 21), (1, 1, 4))),
    (1, 2, 128, 3): ((1, 1, 32), ((1, 1, 32), (1, 1, 10), (1, 1, 2))),
    (1, 2, 192, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 2, 192, 2): ((1, 1, 28), ((1, 1, 28), (1, 1, 9), (1, 1, 1))),
    (1, 2, 192, 3): ((1, 1, 14), ((1, 1, 14), (1, 1, 4), (1, 1, 1))),
    (1, 2, 256, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (1, 2, 256, 2): ((1, 1, 16), ((1, 1, 16), (1, 1, 5), (1, 1, 1))),
    (1, 2, 256, 3): ((1, 1, 8), ((1, 1, 8), (1, 1, 2), (1, 1, 1))),
    (2, 1, 64, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 1, 64, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 42), (1, 1, 8))),
    (2, 1, 64, 3): ((1, 1, 64), ((1, 1, 64), (1, 1, 21), (1, 1, 4))),
    (2, 1, 128, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 1, 128, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 21), (1, 1, 4))),
    (2, 1, 128, 3): ((1, 1, 16), ((1, 1, 16), (1, 1, 5), (1, 1, 1))),
    (2, 1, 192, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 1, 192, 2): ((1, 1, 14), ((1, 1, 14), (1, 1, 4), (1, 1, 1))),
    (2, 1, 192, 3): ((1, 1, 7), ((1, 1, 7), (1, 1, 2), (1, 1, 1))),
    (2, 1, 256, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 1, 256, 2): ((1, 1, 16), ((1, 1, 16), (1, 1, 5), (1, 1, 1))),
    (2, 1, 256, 3): ((1, 1, 4), ((1, 1, 4), (1, 1, 1), (1, 1, 1))),
    (2, 2, 64, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 2, 64, 2): ((1, 1, 64), ((1, 1, 64), (1, 1, 42), (1, 1, 8))),
    (2, 2, 64, 3): ((1, 1, 64), ((1, 1, 64), (1, 1, 21), (1, 1, 4))),
    (2, 2, 128, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 2, 128, 2): ((1, 1, 32), ((1, 1, 32), (1, 1, 10), (1, 1, 2))),
    (2, 2, 128, 3): ((1, 1, 16), ((1, 1, 16), (1, 1, 5), (1, 1, 1))),
    (2, 2, 192, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 2, 192, 2): ((1, 1, 14), ((1, 1, 14), (1, 1, 4), (1, 1, 1))),
    (2, 2, 192, 3): ((1, 1, 7), ((1, 1, 7), (1, 1, 2), (1, 1, 1))),
    (2, 2, 256, 1): ((1, 1, 1), ((1, 1, 1), (1, 1, 1), (1, 1, 1))),
    (2, 2, 256, 2): ((1, 1, 8), ((1, 1, 8), (1, 1, 2), (1, 1, 1))),
    (2, 2, 256, 3): ((1, 1, 4), ((1, 1, 4), (1, 1, 1), (1, 1, 1))),
}


def test_wgrad_splits_table(raw):
    assert len(SPLITS) == 2 * 2 * 4 * 3
    for (n_nets, d_out, hp, nh), (plain, pop) in SPLITS.items():
        got = tuple(raw.nav_mlp_wgrad_splits(n_nets, d_out, hp, nh, M) for M in SPLIT_M)
        assert got == plain, (n_nets, d_out, hp, nh)
        for members, want in zip(SPLIT_MEMBERS, pop):
            got = tuple(raw.nav_mlp_wgrad_splits_pop(members, n_nets, d_out, hp, nh, M)
                        for M in SPLIT_M)
            assert got == want, (members, n_nets, d_out, hp, nh)
