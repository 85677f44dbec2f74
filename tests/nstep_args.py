"""The argument sets nav_nstep_stamp and nav_nstep_rows refuse: one table for the host-side test
(tests/test_nstep_cpu.py: the raw status, dummy pointers) and the device-side one
(tests/test_gpu_nstep.py: live buffers keep their fill)."""
import ctypes as C

import nstep_ref as N
from abi_args import F, Call
from abi_args import v as _v

NAN = float("nan")


def replay(rows=F, capacity=1000):
    from nav._lib import NavReplay
    return lambda: C.byref(NavReplay(rows, capacity))


CALLS = {c.fn: c for c in (
    Call("nav_nstep_stamp", cut=_v(F), capacity=_v(1000), pos=_v(10), n=_v(100), flags=_v(F),
         stream=_v(None)),
    Call("nav_nstep_rows", replay=replay(), cut=_v(F), size=_v(1000), position=_v(300),
         stride=_v(64), n_step=_v(3), gamma=_v(0.99), B=_v(64), idx=_v(None), seed_lo=_v(1),
         seed_hi=_v(2), counter=_v(3), staged=_v(F), steps=_v(None), stream=_v(None)),
)}

BAD = [
    ("nav_nstep_stamp", "NULL cut", dict(cut=_v(None))),
    ("nav_nstep_stamp", "NULL flags", dict(flags=_v(None))),
    ("nav_nstep_stamp", "capacity = 0", dict(capacity=_v(0))),
    ("nav_nstep_stamp", "capacity < 0", dict(capacity=_v(-1))),
    ("nav_nstep_stamp", "n < 0", dict(n=_v(-1))),
    ("nav_nstep_stamp", "n > capacity", dict(n=_v(1001))),
    ("nav_nstep_stamp", "pos < 0", dict(pos=_v(-1))),
    ("nav_nstep_stamp", "pos = capacity", dict(pos=_v(1000))),
    ("nav_nstep_stamp", "pos out of range, n = 0", dict(pos=_v(1000), n=_v(0))),
    ("nav_nstep_rows", "NULL replay", dict(replay=_v(None))),
    ("nav_nstep_rows", "NULL rows", dict(replay=replay(rows=None))),
    ("nav_nstep_rows", "NULL cut", dict(cut=_v(None))),
    ("nav_nstep_rows", "NULL staged", dict(staged=_v(None))),
    ("nav_nstep_rows", "size = 0", dict(size=_v(0), position=_v(0))),
    ("nav_nstep_rows", "size < 0", dict(size=_v(-5))),
    ("nav_nstep_rows", "size > capacity", dict(size=_v(1001))),
    ("nav_nstep_rows", "position < 0", dict(position=_v(-1))),
    ("nav_nstep_rows", "position = capacity", dict(position=_v(1000))),
    ("nav_nstep_rows", "part full, position != size", dict(size=_v(500), position=_v(300))),
    ("nav_nstep_rows", "stride = 0", dict(stride=_v(0))),
    ("nav_nstep_rows", "stride < 0", dict(stride=_v(-64))),
    ("nav_nstep_rows", "n_step = 0", dict(n_step=_v(0))),
    ("nav_nstep_rows", "n_step < 0", dict(n_step=_v(-3))),
    ("nav_nstep_rows", "n_step > NAV_NSTEP_MAX", dict(n_step=_v(N.NSTEP_MAX + 1))),
    ("nav_nstep_rows", "B = 0", dict(B=_v(0))),
    ("nav_nstep_rows", "B < 0", dict(B=_v(-64))),
    ("nav_nstep_rows", "gamma < 0", dict(gamma=_v(-0.01))),
    ("nav_nstep_rows", "gamma > 1", dict(gamma=_v(1.01))),
    ("nav_nstep_rows", "gamma NaN", dict(gamma=_v(NAN))),
]
