"""The demonstrator kernels themselves (csrc/demonstrator.hip: k_rollout, k_cem_rollout,
k_cem_elite, k_demo_augment) against tests/cem_ref.py, the numpy restatement that
tests/test_cem_ref_cpu.py pins to the reference's golden demonstrations: every path, reward, mean,
std and best of every problem, at shapes where workgroups straddle problems, at the kernels' limits
(P = 1, P = 256, E = 1, E = P, T = 0 / 1 / 2, steps = 0, n_aug = 0), with the nullable outputs
absent, and with tied rewards planted where the tie rule (ascending reward, then path index)
decides the elites, their float32 summation order, or best.

Every output buffer carries a sentinel-filled tail of 256 elements that must come back untouched,
and is sentinel-filled before each launch, so a skipped or a stray store shows.

Bounds: exact; 1 float32 ulp for a float32 state against the float32 of the restatement's
free-running f64 state (the kernels' f64 displacement differs from numpy's by ~1e-14, which the
float32 cast can turn into one ulp: tests/test_gpu_dropin.py's bound); 1e-11 for one f64 dynamics
step against the oracle (tests/test_gpu_env.py's bound).

NaN rewards are out of scope: they cannot arise from finite inputs (every state is clipped into
the world and every goal is finite), and the rank rule gives them no defined order.
"""
import numpy as np
import pytest
import torch

import cem_ref
from conftest import golden
from gpu_support import ulps_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 256
HI = cem_ref.HI
SENTINEL = {torch.float32: -777.25, torch.float64: -777.25, torch.int32: -12345}


@pytest.fixture(scope="module")
def env(orc):
    """(lib, speed, angle, device field) on dynamics.npz's field."""
    from nav import _lib
    from nav.vec_env import make_field
    _lib.require_gpu()
    g = golden("dynamics.npz")
    return _lib.lib(), g["speed"], g["angle"], make_field(g["speed"], g["angle"], DEV)


class Out:
    """A sentinel-filled device buffer of n elements plus a TAIL-element tail."""

    def __init__(self, n, dtype):
        self.n, self.sentinel = int(n), SENTINEL[dtype]
        self.t = torch.full((self.n + TAIL,), self.sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        from nav._lib import ptr
        return ptr(self.t)

    def get(self, *shape):
        """The n elements, every one written (no sentinel left), and the tail untouched."""
        h = self.t.cpu().numpy()
        assert np.all(h[self.n:] == self.sentinel), "store past the end"
        assert not np.any(h[:self.n] == self.sentinel), "skipped store"
        return h[:self.n].reshape(shape)


def dev(a, dtype):
    """Input array on the device, padded so that an empty one still has an address."""
    from nav._lib import ptr
    t = torch.zeros(a.size + TAIL, dtype=dtype, device=DEV)
    t[:a.size] = torch.as_tensor(np.ascontiguousarray(a).ravel(), dtype=dtype)
    return t, ptr(t)


def fptr(field):
    from nav._lib import ptr
    return ptr(field)


def stream():
    from nav._lib import stream_handle
    return stream_handle()


# ---------------------------------------------------------------- nav_rollout
@pytest.mark.parametrize("T", [0, 1, 9])
@pytest.mark.parametrize("P", [1, 255, 257])
def test_rollout_every_path_and_reward(env, orc, P, T):
    L, speed, angle, field = env
    rng = np.random.default_rng(1000 * P + T)
    start = rng.uniform(0, HI, (P, 2))
    walls = np.array([[0.0, 0.0], [HI, HI], [0.0, HI], [HI, 0.0], [0.0, 40.5], [63.25, HI]])
    start[:min(P, len(walls))] = walls[(np.arange(min(P, len(walls))) + T) % len(walls)]
    acts = rng.uniform(-7, 7, (P, T, 2))          # beyond +-5: the clip acts
    goal = rng.uniform(5, 95, 2)
    keep = [dev(start, torch.float64), dev(acts, torch.float64), dev(goal, torch.float64)]
    (_, st), (_, ac), (_, gl) = keep
    paths, rew = Out(P * (T + 1) * 2, torch.float64), Out(P, torch.float64)
    L.nav_rollout(fptr(field), P, T, st, ac, paths.ptr, gl, rew.ptr, stream())
    got, r = paths.get(P, T + 1, 2), rew.get(P)
    assert np.array_equal(got[:, 0], start)
    worst = 0.0
    for p in range(P):
        for t in range(T):
            want = orc.dynamics(speed, angle, got[p, t], acts[p, t])   # teacher forced
            worst = max(worst, float(np.abs(got[p, t + 1] - want).max()))
    print("max |step - oracle|", worst)
    assert worst < 1e-11
    assert np.array_equal(r, cem_ref.path_reward(got[:, T], goal))
    # reward = NULL (and goal = NULL): the same paths
    paths2 = Out(P * (T + 1) * 2, torch.float64)
    L.nav_rollout(fptr(field), P, T, st, ac, paths2.ptr, None, None, stream())
    assert np.array_equal(paths2.get(P, T + 1, 2), got)


# ---------------------------------------------------------------- nav_cem_rollout
def cem_inputs(n, P, T, seed):
    """Regions (one touching a wall, one of zero size), uniforms, goals, +-5 first actions,
    normals, and a float32 mean / std with zeros in std and |mean| at and above the +-5 clip."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0, 75, (n, 2))
    region = np.stack([lo[:, 0], lo[:, 0] + 25, lo[:, 1], lo[:, 1] + 25], 1)
    region[0] = [0.0, 25.0, region[0, 2], region[0, 3]]          # touches the wall x = 0
    if n > 1:
        region[1] = [region[1, 0], region[1, 0], region[1, 2], region[1, 2]]   # zero size
    else:
        region[0, 1] = 0.0                                       # zero width, on the wall
    uni = rng.random((n, 2))
    goal = rng.uniform(5, 95, (n, 2))
    a0 = rng.choice([-5.0, 5.0], (n, P, T, 2))
    z = rng.standard_normal((n, P, T, 2))
    mean = (rng.standard_normal((n, T, 2)) * 3).astype(np.float32)
    std = np.abs(rng.standard_normal((n, T, 2))).astype(np.float32)
    flat_m, flat_s = mean.reshape(-1), std.reshape(-1)
    flat_m[0::5] = np.resize(np.array([7.5, -5.0, 5.0, -6.25], np.float32), len(flat_m[0::5]))
    flat_s[0::3] = 0.0
    return region, uni, goal, a0, z, mean, std


def edge_distance(paths):
    """Distance of every state coordinate to the nearest cell edge; a coordinate that sits on the
    clamp (0 or 100 - 1.0001) counts as far (the clamp is exact on both sides)."""
    d = np.abs(paths - np.rint(paths))
    return np.where((paths == 0.0) | (paths == HI), 1.0, d)


CEM_SHAPES = [(1, 1, 1), (3, 40, 5), (7, 37, 12), (2, 256, 3), (5, 100, 7)]


@pytest.mark.parametrize("it", [0, 2])
@pytest.mark.parametrize("n,P,T", CEM_SHAPES)
def test_cem_rollout_every_action_path_and_reward(env, n, P, T, it):
    L, speed, angle, field = env
    region, uni, goal, a0, z, mean, std = cem_inputs(n, P, T, seed=31 * n + 7 * P + T)
    assert (std == 0).any() and (np.abs(mean) >= 5).any()
    ref_a, ref_p, ref_p32, ref_r = cem_ref.cem_rollout(speed, angle, it, region, uni, goal, a0=a0,
                                                       z=z, mean=mean, std=std)
    # precondition on the reference alone: no state so near a cell edge that a 1e-14 difference
    # could pick another cell
    closest = float(edge_distance(ref_p).min())
    print("closest approach to a cell edge", closest)
    assert closest > 1e-9
    # and the 1-ulp bound is relative: a state below 1e-5 that is not exactly 0 has a float32 ulp
    # the size of the f64 difference itself
    assert ref_p[ref_p != 0].min() > 1e-5
    if it:
        assert (np.abs(ref_a) > 5).any()     # stored unclipped
    keep = [dev(x, torch.float64) for x in (region, uni, goal, a0, z)]
    keep += [dev(mean, torch.float32), dev(std, torch.float32)]
    rg, un, gl, a0p, zp, mp, sp = [k[1] for k in keep]
    if it == 0:
        zp = mp = sp = None
    else:
        a0p = None
    N = n * P
    acts, paths, rew = (Out(N * T * 2, torch.float32), Out(N * (T + 1) * 2, torch.float32),
                        Out(N, torch.float64))
    L.nav_cem_rollout(fptr(field), n, P, T, it, rg, un, gl, a0p, zp, mp, sp, acts.ptr,
                      paths.ptr, rew.ptr, stream())
    a, p, r = acts.get(n, P, T, 2), paths.get(n, P, T + 1, 2), rew.get(n, P)
    assert np.array_equal(a, ref_a)
    u = ulps_f32(p, ref_p32)
    print("max path ulps", int(u.max()), "differing states", int((u > 0).sum()))
    assert u.max() <= 1
    # the reward from the device's own float32 final state, exactly
    want_r = cem_ref.path_reward(p[:, :, T].reshape(-1, 2), np.repeat(goal, P, 0)).reshape(n, P)
    assert np.array_equal(r, want_r)
    # paths = NULL: the same actions and rewards
    acts2, rew2 = Out(N * T * 2, torch.float32), Out(N, torch.float64)
    L.nav_cem_rollout(fptr(field), n, P, T, it, rg, un, gl, a0p, zp, mp, sp, acts2.ptr,
                      None, rew2.ptr, stream())
    assert np.array_equal(acts2.get(n, P, T, 2), a)
    assert np.array_equal(rew2.get(n, P), r)


# ---------------------------------------------------------------- nav_cem_elite
ELITE_SHAPES = [(1, 1, 1, 1), (3, 65, 3, 1), (2, 255, 5, 255), (2, 256, 129, 10), (4, 100, 7, 10),
                (3, 64, 1, 64)]


@pytest.mark.parametrize("n,P,T,E", ELITE_SHAPES)
def test_cem_elite_mean_std_best_with_planted_ties(env, n, P, T, E):
    """One launch of distinct rewards, then launches whose problems each carry a different tie
    pattern (cem_ref.tie_patterns) until every pattern the shape has room for has run."""
    L = env[0]
    rng = np.random.default_rng(1000 * P + 10 * T + E)
    pats = [cem_ref.tie_patterns(P, E, rng) for _ in range(n)]
    names = [k for k in pats[0] if k != "distinct"]
    launches = [["distinct"] * n]
    for i in range(0, len(names), n):
        launches.append([names[(i + k) % len(names)] for k in range(n)])
    ran = set()
    for launch in launches:
        rew = np.stack([pats[k][name] for k, name in enumerate(launch)])
        act = (rng.standard_normal((n, P, T, 2)) * 3).astype(np.float32)
        ref = [cem_ref.elite(rew[k], act[k], E) for k in range(n)]
        keep = [dev(rew, torch.float64), dev(act, torch.float32)]
        mean, std, best = (Out(n * T * 2, torch.float32), Out(n * T * 2, torch.float32),
                           Out(n, torch.int32))
        L.nav_cem_elite(n, P, T, E, keep[0][1], keep[1][1], mean.ptr, std.ptr, best.ptr, stream())
        m, s, b = mean.get(n, T, 2), std.get(n, T, 2), best.get(n)
        for k in range(n):
            assert np.array_equal(m[k], ref[k][1]), (launch[k], k)
            assert np.array_equal(s[k], ref[k][2]), (launch[k], k)
            assert b[k] == ref[k][3], (launch[k], k)
        mean2, std2 = Out(n * T * 2, torch.float32), Out(n * T * 2, torch.float32)
        L.nav_cem_elite(n, P, T, E, keep[0][1], keep[1][1], mean2.ptr, std2.ptr, None, stream())
        assert np.array_equal(mean2.get(n, T, 2), m)
        assert np.array_equal(std2.get(n, T, 2), s)
        ran.update(launch)
    assert ran == set(pats[0])


# ---------------------------------------------------------------- the loop
LOOP = dict(T=6, P=33, I=3, E=4)
LOOP_SEED = 7


def corner_problem(speed, angle, P, T, I, rng):
    """A problem whose paths all end in the corner (98.9999, 0): a zero-size region there, the
    goal up-left, and actions that push right and down at every step (the displacement is
    speed * R(rot) a with the corner cell's rot; speed > 0), different for every path. The clamp
    is exact, so every reward is tied in every iteration and the tie rule alone picks the elites."""
    region = np.array([HI, HI, 0.0, 0.0])
    goal = np.array([10.0, 90.0])
    rot = float((np.float32(angle[98, 0]) * np.float32(2.0)) * np.float32(np.pi))
    assert speed[98, 0] > 0

    def into_corner(mag, phi):
        # R(-rot) applied to mag * (cos, sin)(phi), phi around -45 degrees
        return np.stack([mag * np.cos(phi - rot), mag * np.sin(phi - rot)], -1)

    a0 = into_corner(rng.uniform(2, 4, (P, T)), np.deg2rad(rng.uniform(-65, -25, (P, T))))
    z = np.clip(rng.standard_normal((I - 1, P, T, 2)) * 0.25, -0.5, 0.5)
    return region, goal, rng.random(2), a0, z


def loop_inputs(speed, angle):
    T, P, I = LOOP["T"], LOOP["P"], LOOP["I"]
    rng = np.random.default_rng(LOOP_SEED)
    n = 5
    lo = rng.uniform(0, 75, (n, 2))
    region = np.stack([lo[:, 0], lo[:, 0] + 25, lo[:, 1], lo[:, 1] + 25], 1)
    goal = rng.uniform(5, 95, (n, 2))
    uni = rng.random((n, 2))
    a0 = rng.choice([-5.0, 5.0], (n, P, T, 2))
    z = rng.standard_normal((n, I - 1, P, T, 2))
    c = corner_problem(speed, angle, P, T, I, rng)
    return (np.concatenate([region, c[0][None]]), np.concatenate([goal, c[1][None]]),
            np.concatenate([uni, c[2][None]]), np.concatenate([a0, c[3][None]]),
            np.concatenate([z, c[4][None]]))


def test_loop_equals_restatement_and_a_fully_tied_plan(env):
    from nav.cem import batched_demonstrations
    _, speed, angle, field = env
    region, goal, uni, a0, z = loop_inputs(speed, angle)
    ref = cem_ref.demonstrations(speed, angle, region, goal, uni, a0, z, LOOP["E"])
    cem_ref.assert_decisive_gaps(ref["reward"], LOOP["E"])
    assert float(edge_distance(ref["paths"]).min()) > 1e-9
    assert ref["paths"][ref["paths"] != 0].min() > 1e-5
    # the sixth problem: every path in the corner, every reward tied, in every iteration, while
    # its first actions differ from path to path
    assert np.all(ref["paths"][:, 5, :, 1:] == np.array([HI, 0.0]))
    assert np.all(ref["reward"][:, 5] == ref["reward"][0, 5, 0])
    assert len(np.unique(ref["actions"][0, 5].reshape(LOOP["P"], -1), axis=0)) == LOOP["P"]
    assert np.array_equal(ref["order"][:, 5], np.tile(np.arange(LOOP["P"]), (LOOP["I"], 1)))
    st, ac = batched_demonstrations(field, region, goal, uni, a0, z, DEV, **LOOP)
    st, ac = st.cpu().numpy(), ac.cpu().numpy()
    assert st.dtype == ac.dtype == np.float32
    for k in range(6):
        assert np.array_equal(ac[k], ref["plan_actions"][k]), k
        assert ulps_f32(st[k], ref["states"][k]).max() <= 1, k
    assert np.array_equal(st[5], ref["states"][5])     # the clamp is exact


# ---------------------------------------------------------------- nav_demo_augment
AUG_SHAPES = [(1, 2, 0, 1), (3, 5, 2, 0), (2, 3, 1, 2), (4, 7, 4, 3), (1, 40, 4, 3)]


@pytest.mark.parametrize("n_demo,T,steps,n_aug", AUG_SHAPES)
def test_demo_augment_every_point(env, n_demo, T, steps, n_aug):
    L = env[0]
    rng = np.random.default_rng(100 * T + 10 * steps + n_aug)
    states = rng.uniform(0, HI, (n_demo, T, 2)).astype(np.float32)
    D = (T - 1) * (steps + 1) * 4 + 4
    noise = rng.normal(0, 0.1, (n_demo, n_aug, D))
    per = T + n_aug * ((T - 1) * (steps + 1) + 1)
    want = np.stack([cem_ref.augment_points(states[d], noise[d], steps, n_aug)
                     for d in range(n_demo)])
    assert want.shape == (n_demo, per, 2) and want.dtype == np.float64
    keep = [dev(states, torch.float32), dev(noise, torch.float64)]
    out = Out(n_demo * per * 2, torch.float64)
    L.nav_demo_augment(n_demo, T, steps, n_aug, keep[0][1], keep[1][1] if n_aug else None,
                       out.ptr, stream())
    got = out.get(n_demo, per, 2)
    assert got.dtype == np.float64
    assert np.array_equal(got, want)
