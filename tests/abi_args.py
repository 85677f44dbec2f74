"""Calling the C ABI by include/navenv.h's parameter names. What the host-side argument tables
share (tests/test_learner_args_cpu.py, tests/test_env_args_cpu.py and the population tables): the
raw library, the refusal status, a pointer value that is never followed, and a valid argument set
per entry point that a case alters by name; by_name is the same check for a single call (the GPU
launches of tests/launches.py)."""
import ctypes as C
import functools
import os
import subprocess

from conftest import PKG

LIB = os.path.join(PKG, "nav", "libnavenv.so")
EINVAL = -100000
F = 16  # a non-null pointer value that is never dereferenced on the host


def load_raw():
    """The ctypes library with every signature of include/navenv.h set, statuses unchecked."""
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib().raw


SPELLED = {"in": "inp"}  # a header parameter name that Python keeps for itself


@functools.lru_cache(maxsize=None)
def declared(fn):
    """include/navenv.h's parameter names of an entry point, in its order."""
    from nav._abi import parse_header
    return [SPELLED.get(name, name) for _, name in parse_header()[2][fn][1]]


def by_name(lib, fn, **args):
    """One call of a status-returning entry point with every argument given by the header's name,
    in the header's order (a missing, surplus or misplaced name is refused before anything is
    passed); the status must be 0."""
    assert list(args) == declared(fn), (fn, list(args), declared(fn))
    status = getattr(lib, fn)(*args.values())
    assert status == 0, (fn, status)


class Call:
    """A valid argument set of one entry point, by name; a case alters some of them. The names
    are include/navenv.h's parameter names in its order: the arguments are passed by position."""

    def __init__(self, fn, **valid):
        assert list(valid) == declared(fn), (fn, list(valid), declared(fn))
        self.fn, self.valid = fn, valid

    def __call__(self, lib, **changed):
        assert set(changed) <= set(self.valid), changed
        args = {k: (changed[k] if k in changed else v)() for k, v in self.valid.items()}
        return getattr(lib, self.fn)(*args.values())


def v(x):
    return lambda: x


# ---- the population tables: cases alter an Args object (a.m: its nav_td3_member list)
def td3_member(hidden, n_hidden, cap, state_only=False, idx=None):
    """A valid nav_td3_member on the pointer value F: every pointer and both pointer pairs set
    but the nullable idx_critic, idx_actor and eps (idx: values for the two index arrays, as the
    BC entry points want them), the reference's hyper-parameters. state_only: the learner state
    alone (nets, ring, Adam moments) and everything else null, as the exploit entry points read
    a member."""
    from nav._lib import NavMlp, NavReplay, NavTd3Member
    m = NavTd3Member()
    hp = (hidden + 31) // 32 * 32
    net = lambda di, do: NavMlp(di, do, hidden, hp, n_hidden, F, F)  # noqa: E731
    m.actor, m.target_actor = net(2, 2), net(2, 2)
    for i in range(2):
        m.critics[i], m.target_critics[i] = net(4, 1), net(4, 1)
    m.replay = NavReplay(F, cap)
    if state_only:
        m.m_actor = m.v_actor = F
        for i in range(2):
            m.m_critic[i] = m.v_critic[i] = F
        return m
    m.actor_lr, m.critic_lr = 1e-4, 1e-3
    m.policy_noise, m.noise_clip, m.max_action, m.gamma, m.tau = 0.2, 0.5, 5.0, 0.99, 0.005
    for name, kind in m._fields_:
        if kind is C.c_void_p and name not in ("idx_critic", "idx_actor", "eps"):
            setattr(m, name, F)
        elif kind is C.c_void_p * 2:
            getattr(m, name)[0] = getattr(m, name)[1] = F
    if idx is not None:
        m.idx_critic, m.idx_actor = idx
    return m


def set_attr(attr, value):
    def f(a):
        setattr(a, attr, value)
    return f


def member_field(name, value, index=None, m=1):
    def f(a):
        if index is None:
            setattr(a.m[m], name, value)
        else:
            getattr(a.m[m], name)[index] = value
    return f


def net_field(net, field, value, index=None, m=1):
    def f(a):
        d = getattr(a.m[m], net)
        setattr(d if index is None else d[index], field, value)
    return f
