"""What the GPU test modules share that is no launch and no population fixture: the `nav` fixture
(imported by name into each module, so it stays module-scoped there) and the small comparisons."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def nav():
    from nav import _lib
    _lib.require_gpu()
    _lib.lib()
    torch.cuda.set_device(0)
    import nav as navpkg
    return navpkg


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def equal_nan(a, b):
    """Bitwise equality that lets a NaN equal a NaN (prefilled entries a launch leaves alone)."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def ulps_f32(a, b, nonneg=False):
    """|a - b| in f32 steps, for finite floats of one sign (nonneg: asserted finite and
    non-negative)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if nonneg:
        assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def sync_oracle(env, ost):
    """Copy a VecEnv's per-env state into the oracle's VecAgentState (hist is [5][n][2] on the
    device, [n][5][2] in the oracle)."""
    ost.state[:] = env.state.cpu().numpy()
    ost.goal[:] = env.goal.cpu().numpy()
    ost.region[:] = env.region.cpu().numpy()
    ost.hist[:] = env.hist.cpu().numpy().transpose(1, 0, 2)
    ost.meta[:] = env.meta.cpu().numpy().astype(np.uint32)
    ost.plan_index[:] = env.plan_index.cpu().numpy()
    ost.path_length[:] = env.path_length.cpu().numpy()
    ost.episodes[:] = env.episodes.cpu().numpy()
    ost.noise_scale[:] = env.noise_scale.cpu().numpy()
