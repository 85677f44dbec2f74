"""nav_test_rollout's host-side argument validation: every bad call returns NAV_EINVAL before any
launch, and n = 0 is a no-op (no kernel is launched by these calls, so no GPU is needed)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "nav", "libnavenv.so")
FAKE = 16  # a non-null pointer value that is never dereferenced on the host


@pytest.fixture(scope="module")
def navlib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j4", "-C", PKG], check=True)
    from nav import _lib
    return _lib.lib()


def soa(n, goal=FAKE, region=FAKE):
    from nav._lib import NavEnvSoa
    return NavEnvSoa(n, FAKE, goal, region, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)


def test_binding_declares_the_entry_point():
    from nav._lib import SIGNATURES, NavTestOut
    assert "nav_test_rollout" in {s[0] for s in SIGNATURES}
    assert [f[0] for f in NavTestOut._fields_] == ["reached", "steps", "best_distance",
                                                   "final_state", "traj"]


def test_host_validation(navlib):
    from nav._lib import NavError, NavMlp, NavTestOut, params_struct
    p = params_struct()
    actor = NavMlp(2, 2, 256, 256, 2, FAKE, FAKE)
    out = NavTestOut(FAKE, FAKE, FAKE, FAKE, None)  # traj is nullable
    env = soa(97)

    def call(p_=p, actor_=actor, env_=env, field=FAKE, start=None, max_steps=10, out_=out):
        ref = lambda x: None if x is None else C.byref(x)
        return navlib.nav_test_rollout(ref(p_), ref(actor_), ref(env_), field, start, 0,
                                       max_steps, ref(out_), None)

    def bad(**kw):
        with pytest.raises(NavError, match="invalid argument"):
            call(**kw)

    # null p / actor / env / field / out
    bad(p_=None)
    bad(actor_=None)
    bad(env_=None)
    bad(field=None)
    bad(out_=None)
    # every non-nullable output pointer
    for k in range(4):
        ptrs = [FAKE] * 4 + [FAKE]
        ptrs[k] = None
        bad(out_=NavTestOut(*ptrs))
    # an actor that is not 2 -> 2
    bad(actor_=NavMlp(4, 1, 256, 256, 2, FAKE, FAKE))
    bad(actor_=NavMlp(2, 1, 256, 256, 2, FAKE, FAKE))
    bad(actor_=NavMlp(2, 2, 200, 200, 3, FAKE, FAKE))  # hidden width not padded to 32
    # max_steps outside 1 .. 1 << 20
    bad(max_steps=0)
    bad(max_steps=-1)
    bad(max_steps=(1 << 20) + 1)
    # n < 0 and n >= 2^31
    bad(env_=soa(-1))
    bad(env_=soa(1 << 31))
    # the goals always, the regions when the starts are drawn
    bad(env_=soa(97, goal=None))
    bad(env_=soa(97, region=None))
    bad(env_=soa(97, goal=None), start=FAKE)
    # n = 0: no-op, whatever the per-env pointers are
    assert call(env_=soa(0, goal=None, region=None)) == 0
    assert call(env_=soa(0), out_=NavTestOut(None, None, None, None, None), max_steps=1 << 20) == 0
