"""What the host-side argument tables of the C ABI share (tests/test_learner_args_cpu.py,
tests/test_env_args_cpu.py): the raw library, the refusal status, a pointer value that is never
followed, and a valid argument set per entry point that a case alters by name."""
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


class Call:
    """A valid argument set of one entry point, by name; a case alters some of them. The names
    are include/navenv.h's parameter names in its order: the arguments are passed by position."""

    def __init__(self, fn, **valid):
        from nav._abi import parse_header
        declared = [SPELLED.get(name, name) for _, name in parse_header()[2][fn][1]]
        assert list(valid) == declared, (fn, list(valid), declared)
        self.fn, self.valid = fn, valid

    def __call__(self, lib, **changed):
        assert set(changed) <= set(self.valid), changed
        args = {k: (changed[k] if k in changed else v)() for k, v in self.valid.items()}
        return getattr(lib, self.fn)(*args.values())


def v(x):
    return lambda: x
