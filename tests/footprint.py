"""Memory-footprint checker for a launch: where it stores, what it leaves alone, and whether its
result depends on what its outputs held before.

A launch under test gets every pointer argument as a window (`Win`) inside a larger buffer,

    [ guard | n elements | guard ]

and runs twice from identical inputs, once per fill. Run A fills every guard and every `out`
window with the float32 signalling-NaN pattern 0x7FA5C3E1 (integer types: the byte 0xA5), run B
with 0x4E6E6B28 = 1e9f (integer types: the byte 0x5A); the guards of `in` and `inout` windows
carry the same fill. float64 windows take the analogous pair: the signalling NaN
0x7FF4A5C3E1A5C3E1 and 1e9. A third run uses ordinary exact-size zeroed allocations, as every other
test of the suite does. `check` then asserts, byte for byte and without tolerances:

 1. stray store           every guard of every window is unchanged in both runs;
 2. input preserved       every `in` window is unchanged in both runs;
 3. written set           the elements of an `out` window that still hold the fill in BOTH runs
                          are exactly the expected untouched set of that window (closed form, from
                          include/navenv.h); every other element was written;
 4. no dependence on      outside the expected untouched set, runs A and B give bit-identical
    prior contents        `out` and `inout` results, and run A's float results are finite: an
                          accumulate-into-output, a read of an unwritten workspace or an over-read
                          of an input's slack that reaches an output shows here (NaN + x is a quiet
                          NaN, 1e9 + x is not the fill);
 5. same result as today  run A equals the zero-allocation run bit for bit, so this harness cannot
                          drift from what the other tests pin.

The guard is max(4096, 64 * row pitch in bytes) rounded up to 256 bytes: one stray 64-row tile of
the buffer's own row pitch stays inside it (a derived number: the tallest row workgroup holds 64
rows). The window's first element is 256-byte aligned, so float4 access stays legal.

What this method cannot see: an over-read that never reaches an output (a load past an input
whose value is then discarded), and a store of more than one guard past a window.

The module needs numpy only; `TorchMem` imports torch when it is used. tests/test_footprint_cpu.py
drives it with numpy fakes on `HostMem` to show that each kind of wrong launch is caught.
"""
import ctypes as C

import numpy as np

ROLES = ("in", "out", "inout")
FILL_F32 = {"A": 0x7FA5C3E1, "B": 0x4E6E6B28}
FILL_F64 = {"A": 0x7FF4A5C3E1A5C3E1, "B": int(np.float64(1e9).view(np.uint64))}
FILL_BYTE = {"A": 0xA5, "B": 0x5A}
ALIGN = 256
TILE_ROWS = 64

# the named causes, in the order the checks run
STRAY = "stray store"
INPUT = "input modified"
SKIPPED = "untouched outside the expected set"
OVERWRITTEN = "written inside the expected untouched set"
PRIOR = "depends on prior contents"
NONFINITE = "non-finite output"
DRIFT = "differs from the zero-allocation run"


class FootprintError(AssertionError):
    def __init__(self, findings):
        self.findings = findings
        self.causes = [f[0] for f in findings]
        super().__init__("; ".join(f"{c}: {d}" for c, d in findings))


def guard_bytes(pitch_bytes):
    """max(4096, 64 rows of the buffer's pitch), rounded up to 256."""
    g = max(4096, TILE_ROWS * int(pitch_bytes))
    return (g + ALIGN - 1) // ALIGN * ALIGN


def fill_pattern(dtype, run):
    """The fill of one element of `dtype` in run 'A' or 'B', as an array of its bytes."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([FILL_F32[run]], np.uint32).view(np.uint8)
    if dtype == np.float64:
        return np.array([FILL_F64[run]], np.uint64).view(np.uint8)
    assert dtype.kind in "iu", dtype
    return np.full(dtype.itemsize, FILL_BYTE[run], np.uint8)


class Win:
    """A window of n elements of `dtype`; role 'in' / 'inout' windows carry their initial
    contents `init` (n elements), pitch = the buffer's row pitch in elements."""

    def __init__(self, n, dtype, role, pitch=None, init=None):
        assert role in ROLES, role
        self.n, self.dtype, self.role = int(n), np.dtype(dtype), role
        assert self.n >= 1
        self.pitch = int(pitch) if pitch else 1
        self.guard = guard_bytes(self.pitch * self.dtype.itemsize)
        self.nbytes = self.n * self.dtype.itemsize
        if role == "out":
            assert init is None
            self.init = None
        else:
            a = np.ascontiguousarray(init).reshape(-1)
            assert a.size == self.n, (a.size, self.n)
            self.init = a.astype(self.dtype, copy=True) if a.dtype != self.dtype else a.copy()
            self.init.setflags(write=False)

    def image(self, run):
        """Host image [guard | body | guard] of run 'A' / 'B' as bytes."""
        pat = fill_pattern(self.dtype, run)
        img = np.tile(pat, (2 * self.guard + self.nbytes) // pat.size)
        if self.init is not None:
            img[self.guard:self.guard + self.nbytes] = self.init.view(np.uint8)
        return img

    def plain(self):
        """The exact-size zero allocation's contents."""
        img = np.zeros(self.nbytes, np.uint8)
        if self.init is not None:
            img[:] = self.init.view(np.uint8)
        return img


class HostMem:
    """numpy-backed memory for the fakes of tests/test_footprint_cpu.py."""

    def alloc(self, nbytes):
        raw = np.zeros(nbytes + ALIGN, np.uint8)
        off = (-raw.ctypes.data) % ALIGN
        return raw, raw[off:off + nbytes], raw.ctypes.data + off

    def upload(self, view, img):
        view[:] = img

    def download(self, view):
        return view.copy()

    def sync(self):
        pass


class TorchMem:
    """Device memory: one uint8 tensor per window."""

    def __init__(self, device="cuda"):
        import torch
        self.torch, self.device = torch, device

    def alloc(self, nbytes):
        raw = self.torch.empty(nbytes + ALIGN, dtype=self.torch.uint8, device=self.device)
        off = (-raw.data_ptr()) % ALIGN
        return raw, raw[off:off + nbytes], raw.data_ptr() + off

    def alloc_zero(self, nbytes):
        """An ordinary allocation of its exact size, as the rest of the suite makes them."""
        raw = self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.device)
        return raw, raw, raw.data_ptr()

    def upload(self, view, img):
        view.copy_(self.torch.from_numpy(img))

    def download(self, view):
        return view.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()


class Bound:
    """A window placed in memory for one run: `addr` / `ptr` of its first element. On HostMem,
    `view` is the numpy array of the n elements and `raw` the typed array of the whole buffer with
    the window at raw[lo : lo + n] (the fakes stray through it)."""

    def __init__(self, win, mem, run):
        self.win, self.mem, self.run = win, mem, run
        if run == "plain":
            alloc = getattr(mem, "alloc_zero", None)
            if alloc is None:
                self.keep, self.bytes, base = mem.alloc(win.nbytes)
            else:
                self.keep, self.bytes, base = alloc(win.nbytes)
            self.addr = base
            mem.upload(self.bytes, win.plain())
            lo_bytes = 0
        else:
            self.keep, self.bytes, base = mem.alloc(2 * win.guard + win.nbytes)
            self.addr = base + win.guard
            mem.upload(self.bytes, win.image(run))
            lo_bytes = win.guard
        assert self.addr % ALIGN == 0 or run == "plain"
        self.ptr = C.c_void_p(self.addr)
        if isinstance(self.bytes, np.ndarray):
            self.raw = self.bytes.view(win.dtype)
            self.lo = lo_bytes // win.dtype.itemsize
            self.view = self.raw[self.lo:self.lo + win.n]

    def snapshot(self):
        """(guard before, body as uint8, guard after) on the host."""
        h = self.mem.download(self.bytes)
        g = 0 if self.run == "plain" else self.win.guard
        return h[:g], h[g:g + self.win.nbytes], h[g + self.win.nbytes:]


def bind(wins, mem, run):
    return {name: Bound(w, mem, run) for name, w in wins.items()}


def _where(bad, limit=6):
    idx = np.flatnonzero(bad)
    return f"{idx.size} element(s), first at {idx[:limit].tolist()}"


def _elem_ne(a, b, itemsize):
    """Per element: do the byte images differ."""
    u = np.dtype(f"u{itemsize}")
    return np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)


def check(launch, wins, untouched=None, mem=None, collect=False):
    """Run `launch(bound)` (bound: name -> Bound) under both fills and on zero allocations and
    apply the five checks. `untouched`: name -> bool array [n] (True = expected untouched) for the
    `out` windows that are not written in full. Raises FootprintError naming every cause found
    (collect=True: returns them beside the values instead). Returns run A's windows as typed host
    arrays, name -> array [n]."""
    mem = mem or TorchMem()
    untouched = untouched or {}
    for name in untouched:
        assert wins[name].role == "out", f"{name}: an expected untouched set needs an out window"
    findings, snaps, skipped = [], {}, {}
    for run in ("A", "B"):
        bound = bind(wins, mem, run)
        launch(bound)
        mem.sync()
        snaps[run] = {name: b.snapshot() for name, b in bound.items()}
        del bound
    expect = {}
    for name, w in wins.items():
        size = w.dtype.itemsize
        # 1. stray store
        for run in ("A", "B"):
            pat = fill_pattern(w.dtype, run)
            for side, g in (("before", snaps[run][name][0]), ("after", snaps[run][name][2])):
                bad = g.reshape(-1, pat.size) != pat
                if bad.any():
                    at = np.flatnonzero(bad.any(axis=1))
                    at = at - g.size // pat.size if side == "before" else at + w.n
                    findings.append((STRAY, f"{name} run {run}: guard {side} the window changed at "
                                            f"element {at[:6].tolist()} ({at.size} in all)"))
        bodyA, bodyB = snaps["A"][name][1], snaps["B"][name][1]
        exp = np.zeros(w.n, bool)
        if name in untouched:
            exp = np.asarray(untouched[name], bool).reshape(-1)
            assert exp.size == w.n, (name, exp.size, w.n)
        expect[name] = exp
        if w.role == "in":
            # 2. input preserved
            init = w.init.view(np.uint8)
            for run, body in (("A", bodyA), ("B", bodyB)):
                bad = _elem_ne(body, init, size)
                if bad.any():
                    findings.append((INPUT, f"{name} run {run}: {_where(bad)}"))
            continue
        if w.role == "out":
            # 3. written set
            kept = ~_elem_ne(bodyA, np.tile(fill_pattern(w.dtype, "A"), w.n), size) & \
                   ~_elem_ne(bodyB, np.tile(fill_pattern(w.dtype, "B"), w.n), size)
            if (kept & ~exp).any():
                findings.append((SKIPPED, f"{name}: {_where(kept & ~exp)}"))
            if (exp & ~kept).any():
                findings.append((OVERWRITTEN, f"{name}: {_where(exp & ~kept)}"))
        # 4. no dependence on prior contents (an unwritten element is check 3's finding alone)
        bad = _elem_ne(bodyA, bodyB, size) & ~exp
        if w.role == "out":
            bad &= ~kept
            skipped[name] = kept & ~exp
        if bad.any():
            findings.append((PRIOR, f"{name}: runs A and B differ at {_where(bad)}"))
        if w.dtype.kind == "f":
            bad = ~np.isfinite(bodyA.view(w.dtype)) & ~exp
            if w.role == "out":
                bad &= ~kept
            if bad.any():
                findings.append((NONFINITE, f"{name} run A: {_where(bad)}"))
    # 5. same result as the zero-allocation run (never after a stray store: the exact-size
    # allocations have no guard to catch it)
    if STRAY not in [f[0] for f in findings]:
        bound = bind(wins, mem, "plain")
        launch(bound)
        mem.sync()
        for name, w in wins.items():
            if w.role == "in":
                continue
            bad = _elem_ne(snaps["A"][name][1], bound[name].snapshot()[1], w.dtype.itemsize)
            bad &= ~expect[name]
            if name in skipped:
                bad &= ~skipped[name]
            if bad.any():
                findings.append((DRIFT, f"{name}: {_where(bad)}"))
        del bound
    values = {name: np.ascontiguousarray(snaps["A"][name][1]).view(w.dtype)
              for name, w in wins.items()}
    if collect:
        return findings, values
    if findings:
        raise FootprintError(findings)
    return values
