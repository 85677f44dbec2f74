"""tests/footprint.py can fail: numpy fake launches on host buffers, one well behaved and one per
kind of wrong store, each of which must make the checker raise with its own named cause. This is
what shows that tests/test_gpu_footprint.py would fail on a subtly wrong kernel; nothing is
provoked on a GPU, and no library is loaded.

The fake is a strided copy out[r][2 + j] = 2 * x[r][j] + w[j] of ROWS x 3 values into rows of
pitch 8 (so columns 0, 1 and 5 .. 7 are the expected untouched set), plus a counter `acc` that the
launch increments (an inout window)."""
import numpy as np
import pytest

import footprint as F

ROWS, COLS, LD, COL0 = 37, 3, 8, 2


def _wins():
    rng = np.random.default_rng(7)
    x = rng.uniform(1000, 2000, (ROWS, COLS)).astype(np.float32)
    w = rng.uniform(1000, 2000, COLS).astype(np.float32)
    return {"x": F.Win(ROWS * COLS, np.float32, "in", pitch=COLS, init=x),
            "w": F.Win(COLS, np.float32, "in", init=w),
            "idx": F.Win(ROWS, np.int64, "in", init=np.arange(ROWS)),
            "out": F.Win(ROWS * LD, np.float32, "out", pitch=LD),
            "cnt": F.Win(ROWS, np.int32, "out"),
            "acc": F.Win(4, np.float64, "inout", init=[1.0, 2.0, 3.0, 4.0])}


def _untouched():
    m = np.ones((ROWS, LD), bool)
    m[:, COL0:COL0 + COLS] = False
    return {"out": m}


def good(b, rows=ROWS, accumulate=False, cols=range(COLS)):
    x = b["x"].view.reshape(ROWS, COLS)
    out = b["out"].view.reshape(ROWS, LD)
    for j in cols:
        v = 2 * x[:rows, j] + b["w"].view[j]
        if accumulate:
            with np.errstate(invalid="ignore"):
                out[:rows, COL0 + j] += v
        else:
            out[:rows, COL0 + j] = v
    b["cnt"].view[:] = b["idx"].view[:] + 1
    b["acc"].view[:] += 1.0


def run(launch, **kw):
    return F.check(launch, _wins(), _untouched(), mem=F.HostMem(), **kw)


def test_guard_and_alignment_rules():
    assert F.guard_bytes(4) == 4096                       # small pitch: the 4 KiB floor
    assert F.guard_bytes(64) == 4096                      # 64 rows x 64 B, exactly the floor
    assert F.guard_bytes(224 * 4) == 64 * 224 * 4         # one 64-row tile of the row pitch
    assert F.guard_bytes(65) == 4352                      # 64 x 65 B = 4160, rounded up to 256
    assert F.Win(10, np.uint8, "out", pitch=65).guard == 4352
    mem = F.HostMem()
    for name, w in _wins().items():
        assert w.guard == F.guard_bytes(w.pitch * w.dtype.itemsize) and w.guard % 256 == 0
        for tag in ("A", "B"):
            b = F.Bound(w, mem, tag)
            assert b.addr % 256 == 0, name
            assert b.view.ctypes.data == b.addr and b.view.size == w.n
            before, body, after = b.snapshot()
            assert before.size == after.size == w.guard and body.size == w.nbytes
            pat = F.fill_pattern(w.dtype, tag)
            assert (before.reshape(-1, pat.size) == pat).all()
            assert (after.reshape(-1, pat.size) == pat).all()
            if w.role == "out":
                assert (body.reshape(-1, pat.size) == pat).all()
            else:
                assert np.array_equal(body.view(w.dtype), w.init)


def test_fill_patterns():
    a = F.fill_pattern(np.float32, "A").view(np.uint32)[0]
    assert a == 0x7FA5C3E1 and np.isnan(F.fill_pattern(np.float32, "A").view(np.float32)[0])
    assert a & 0x00400000 == 0                            # signalling: arithmetic changes it
    assert F.fill_pattern(np.float32, "B").view(np.float32)[0] == np.float32(1e9)
    assert F.fill_pattern(np.float32, "B").view(np.uint32)[0] == 0x4E6E6B28
    assert np.isnan(F.fill_pattern(np.float64, "A").view(np.float64)[0])
    assert F.fill_pattern(np.float64, "B").view(np.float64)[0] == 1e9
    for dt in (np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64):
        assert (F.fill_pattern(dt, "A") == 0xA5).all() and (F.fill_pattern(dt, "B") == 0x5A).all()
        assert F.fill_pattern(dt, "A").size == np.dtype(dt).itemsize


def test_well_behaved_launch_passes():
    vals = run(good)
    w = _wins()
    want = 2 * w["x"].init.reshape(ROWS, COLS) + w["w"].init
    assert np.array_equal(vals["out"].reshape(ROWS, LD)[:, COL0:COL0 + COLS], want)
    assert np.array_equal(vals["acc"], [2.0, 3.0, 4.0, 5.0])
    findings, _ = run(good, collect=True)
    assert findings == []


def _raises(launch, cause, where=None):
    with pytest.raises(F.FootprintError) as e:
        run(launch)
    assert cause in e.value.causes, e.value.causes
    if where:
        assert any(c == cause and where in d for c, d in e.value.findings), e.value.findings
    return e.value


def test_store_one_past_the_end():
    def bad(b):
        good(b)
        o = b["out"]
        o.raw[o.lo + o.win.n] = 1.0
    _raises(bad, F.STRAY, f"guard after the window changed at element [{ROWS * LD}]")


def test_store_one_before_the_start():
    def bad(b):
        good(b)
        c = b["cnt"]
        c.raw[c.lo - 1] = 0
    _raises(bad, F.STRAY, "cnt run A: guard before the window changed at element [-1]")


def test_stray_store_skips_the_zero_allocation_run():
    calls = []

    def bad(b):
        calls.append(b["out"].run)
        good(b)
        if b["out"].run != "plain":
            b["out"].raw[b["out"].lo + b["out"].win.n] = 1.0
    _raises(bad, F.STRAY)
    assert calls == ["A", "B"]


def test_skipped_last_row():
    e = _raises(lambda b: good(b, rows=ROWS - 1), F.SKIPPED,
                f"out: {COLS} element(s), first at "
                f"{[(ROWS - 1) * LD + COL0 + j for j in range(COLS)]}")
    assert set(e.causes) == {F.SKIPPED}   # the unwritten elements are this check's finding alone


def test_accumulate_instead_of_store():
    e = _raises(lambda b: good(b, accumulate=True), F.PRIOR, "out")
    assert F.SKIPPED not in e.causes     # the elements were written: the fill did not survive


def test_modified_input():
    def bad(b):
        good(b)
        b["idx"].view[5] = 4
    _raises(bad, F.INPUT, "idx run A: 1 element(s), first at [5]")


def test_result_depends_on_the_slack_after_an_input():
    def bad(b):
        good(b)
        x = b["x"]
        # row ROWS of x (an exact-size allocation has no such element: the fake reads 0 there)
        over = x.raw[x.lo + x.win.n] if x.run != "plain" else np.float32(0)
        with np.errstate(invalid="ignore"):
            b["out"].view.reshape(ROWS, LD)[ROWS - 1, COL0] += over
    _raises(bad, F.PRIOR, f"out: runs A and B differ at 1 element(s), first at "
                          f"[{(ROWS - 1) * LD + COL0}]")


def test_untouched_element_outside_the_expected_set():
    _raises(lambda b: good(b, cols=(0, 2)), F.SKIPPED,
            f"out: {ROWS} element(s), first at {[r * LD + COL0 + 1 for r in range(6)]}")


def test_written_element_inside_the_expected_untouched_set():
    def bad(b):
        good(b)
        b["out"].view.reshape(ROWS, LD)[3, 0] = 0.0      # a padded column
    _raises(bad, F.OVERWRITTEN, f"out: 1 element(s), first at [{3 * LD}]")


def test_differs_from_the_zero_allocation_run():
    """A launch that behaves differently on exact-size allocations: check 5."""
    def bad(b):
        good(b)
        if b["out"].run == "plain":
            b["out"].view[COL0] = -1.0
    _raises(bad, F.DRIFT, f"out: 1 element(s), first at [{COL0}]")


def test_non_finite_output():
    def bad(b):
        good(b)
        b["out"].view[COL0] = np.inf
    _raises(bad, F.NONFINITE, f"out run A: 1 element(s), first at [{COL0}]")
