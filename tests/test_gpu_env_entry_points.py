"""The entry points of the environment units that no other GPU test reaches (Robot.check_if_stuck
and Robot.compute_reward have no caller among them, and the package pools its events instead of
destroying them), called through the raw C ABI at 65 items: a full wave plus one lane.

Both oracle functions are the same f64 expressions as the kernels (norm2 with its fma, the
squared distance without, one correctly rounded sqrt; the oracle is built with
-ffp-contract=off), so the comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_support import nav  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 65


def test_check_if_stuck_vs_oracle(nav, orc):
    """nav_check_if_stuck over 14 calls: a third of the envs stand still (stuck on the sixth call,
    history cleared, stuck again six calls later), a third creep by 0.3 * (1, 1) per call (the
    oldest of five states is 2.12 away: never stuck, the ring's head advances), a third jump by
    3. Every call's verdict and the final count / head bits of meta against orc_check_if_stuck."""
    from nav._lib import NavEnvSoa, lib, params_struct, ptr, stream_handle
    p = params_struct()
    hist = torch.zeros(5, N, 2, dtype=torch.float64, device=DEV)
    meta = torch.full((N,), 5, dtype=torch.int32, device=DEV)  # low byte: kept as it is
    soa = NavEnvSoa(n=N, hist=hist.data_ptr(), meta=meta.data_ptr())
    stuck = torch.zeros(N, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(7)
    start = rng.uniform(10.0, 50.0, (N, 2))
    drift = np.array([0.0, 0.3, 3.0])[np.arange(N) % 3][:, None] * np.ones(2)
    ref = [orc.StuckHistory() for _ in range(N)]
    fired = 0
    for t in range(14):
        s = start + drift * t
        st = torch.tensor(s, device=DEV)
        lib().nav_check_if_stuck(C.byref(p), C.byref(soa), ptr(st), ptr(stuck), stream_handle())
        want = np.array([ref[e].check(s[e], p.stuck_threshold) for e in range(N)])
        assert np.array_equal(stuck.cpu().numpy().astype(bool), want), t
        fired += int(want.sum())
    assert fired == 2 * len(range(0, N, 3))
    m = meta.cpu().numpy()
    assert np.all((m & 0xff) == 5)
    assert np.array_equal((m >> 8) & 7, [r.count.value for r in ref])
    assert np.array_equal((m >> 12) & 7, [r.head.value for r in ref])


@pytest.mark.parametrize("m", [1, 7])
def test_demo_min_vs_oracle(nav, orc, m):
    from nav._lib import lib, ptr, stream_handle
    rng = np.random.default_rng(11 + m)
    pts = rng.uniform(-5.0, 105.0, (N, 2))
    demo = rng.uniform(0.0, 100.0, (m, 2))
    pts[3] = demo[0]  # a distance of exactly 0
    out = torch.full((N,), -1.0, dtype=torch.float64, device=DEV)
    d_pts, d_demo = torch.tensor(pts, device=DEV), torch.tensor(demo, device=DEV)
    lib().nav_demo_min(ptr(d_pts), N, ptr(d_demo), m, ptr(out), stream_handle())
    want = np.array([orc.demo_min(demo, x, y) for x, y in pts])
    assert np.array_equal(out.cpu().numpy(), want)


def test_event_create_record_elapsed_destroy(nav):
    from nav._lib import lib, stream_handle
    a, b = C.c_void_p(), C.c_void_p()
    lib().nav_event_create(C.byref(a))
    lib().nav_event_create(C.byref(b))
    assert a.value and b.value and a.value != b.value
    lib().nav_event_record(a, stream_handle())
    torch.zeros(1 << 20, device=DEV).sum()
    lib().nav_event_record(b, stream_handle())
    ms = C.c_float(-1.0)
    lib().nav_event_elapsed_ms(a, b, C.byref(ms))
    assert 0.0 <= ms.value < 1e4
    assert lib().nav_event_destroy(a) == 0 and lib().nav_event_destroy(b) == 0
