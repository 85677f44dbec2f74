"""Multi-step returns, host side: the restatement tests/nstep_ref.py against a hand-worked ring,
a brute-force discounted sum and itself; the coverage of the kernel tests' seeded cases; the
argument sets nav_nstep_stamp and nav_nstep_rows refuse with the raw status NAV_EINVAL before any
HIP call (no kernel is launched, the dummy pointers are never followed, so no GPU is needed); and
the refusals of the config, the learner, the trainer and the population that need no device."""
import collections

import numpy as np
import pytest

import nstep_ref as N
from abi_args import EINVAL, load_raw
from abi_args import v as _v
from nstep_args import BAD, CALLS

SEED = 1707366464


# ---- the restatement
def hand_ring():
    """12 rows, 3 envs (stride 3), full, the write head at slot 2: the ticks wrote rows (2 3 4),
    (5 6 7), (8 9 10), (11 0 1). Env 0 owns rows 2 5 8 11 (its path ended at row 5: done and cut),
    env 1 rows 3 6 9 0 (nothing ended), env 2 rows 4 7 10 1 (reset without done after row 7).
    Row k: s = (k, -k), a = (10 k, -10 k), r = (-1)^k (k + 1), s' = (100 + k, 200 + k)."""
    ring = np.zeros((12, 8), np.float32)
    for k in range(12):
        ring[k] = (k, -k, 10 * k, -10 * k, (-1) ** k * (k + 1), 100 + k, 200 + k, 0)
    ring[5, 7] = 1
    cut = np.zeros(12, np.uint8)
    cut[[5, 7]] = 1
    return ring, cut


# k0: (horizon, R at gamma 0.5, the last row, column 7) worked by hand; r_k = (-1)^k (k + 1)
HAND = {
    0: (1, 1.0, 0, 0.0),                          # one row below the write head
    1: (1, -2.0, 1, 0.0),                         # the newest row
    2: (2, 3 + 0.5 * -6, 5, 1.0),                 # done in the middle: the bootstrap is off
    3: (3, -4 + 0.5 * 7 + 0.25 * -10, 9, 0.75),   # n_step reached
    4: (2, 5 + 0.5 * -8, 7, 0.5),                 # cut in the middle, no done
    5: (1, -6.0, 5, 1.0),                         # cut (and done) at the first row
    6: (3, 7 + 0.5 * -10 + 0.25 * 1, 0, 0.75),    # n_step reached through slot 0
    7: (1, -8.0, 7, 0.0),                         # cut at the first row, no done
    8: (2, 9 + 0.5 * -12, 11, 0.5),               # the write head after two rows
    9: (2, -10 + 0.5 * 1, 0, 0.5),                # the write head, the chain wrapped to slot 0
    10: (2, 11 + 0.5 * -2, 1, 0.5),               # the write head, the chain wrapped to slot 1
    11: (1, -12.0, 11, 0.0),                      # the write head at once
}
HAND_CAUSES = {0: "head", 1: "head", 2: "done", 3: "n_step", 4: "cut", 5: "done", 6: "n_step",
               7: "cut", 8: "head", 9: "head", 10: "head", 11: "head"}


def test_hand_worked_ring():
    ring, cut = hand_ring()
    causes = []
    staged, steps = N.rows(ring, cut, 12, 2, 3, 3, 0.5, np.arange(12), causes)
    for k0, (m, R, last, d7) in HAND.items():
        assert steps[k0] == m, k0
        want = np.array([*ring[k0, :4], R, 100 + last, 200 + last, d7], np.float32)
        assert np.array_equal(staged[k0].view(np.uint32), want.view(np.uint32)), (k0, staged[k0])
        assert causes[k0] == HAND_CAUSES[k0], k0
    # the discount the critic kernel applies: gamma^m exactly at gamma = 0.5, 0 after done
    disc = N.discount(staged, 0.5)
    for k0, (m, _, _, d7) in HAND.items():
        assert disc[k0] == (0.0 if d7 == 1.0 else 0.5 ** m), k0
    # a horizon of 1 is the ring's own row
    one = steps == 1
    assert one.sum() == 5 and np.array_equal(staged[one].view(np.uint32),
                                             ring[one].view(np.uint32))
    # n_step = 2 ends rows 3 and 6 one row earlier and changes no other
    staged2, steps2 = N.rows(ring, cut, 12, 2, 3, 2, 0.5, np.arange(12))
    assert steps2.tolist() == [min(m, 2) for m in steps.tolist()]
    same = steps <= 2
    assert np.array_equal(staged2[same].view(np.uint32), staged[same].view(np.uint32))
    assert staged2[3].tolist() == [3, -3, 30, -30, -4 + 3.5, 106, 206, 0.5]


def test_sum_equals_the_brute_force_discounted_return():
    """Simulated episodes of 5 envs for 40 ticks, no cut and no wrap (a part-full ring): R is the
    env's discounted reward sum in fp64 (powers by pow, not by repeated multiplication) to 1 ulp
    of f32, with the horizon cut only by the write head."""
    n_envs, T, cap, n_step = 5, 40, 256, 8
    rng = np.random.default_rng(7)
    rew = (rng.standard_normal((T, n_envs)) * 20).astype(np.float32)
    ring = np.zeros((cap, 8), np.float32)
    ring[:T * n_envs] = rng.standard_normal((T * n_envs, 8)).astype(np.float32)
    ring[:, 7] = 0
    ring[:T * n_envs, 4] = rew.reshape(-1)
    cut = np.zeros(cap, np.uint8)
    size = T * n_envs
    g32 = np.float32(0.99)
    staged, steps = N.rows(ring, cut, size, size, n_envs, n_step, g32, np.arange(size))
    worst = 0.0
    for k0 in range(size):
        t, e = divmod(k0, n_envs)
        m = min(n_step, T - t)
        assert steps[k0] == m, k0
        ref = sum(np.float64(g32) ** j * np.float64(rew[t + j, e]) for j in range(m))
        err = abs(float(staged[k0, 4]) - ref) / np.spacing(np.float32(abs(ref)))
        worst = max(worst, err)
        last = k0 + (m - 1) * n_envs
        assert np.array_equal(staged[k0, 5:7], ring[last, 5:7])
        assert abs(float(staged[k0, 7]) - (1 - float(g32) ** (m - 1))) <= 2.0 ** -24
        # the applied discount: within one f32 rounding of gamma^m (and the rounding of 1 - g^(m-1))
        d = float(N.discount(staged[k0:k0 + 1], g32)[0])
        assert abs(d - float(g32) ** m) <= 2 * 2.0 ** -24, (k0, m)
    print(f"max |R - brute force| {worst:.3f} ulp of f32")
    assert worst <= 1.0


@pytest.mark.parametrize("capacity,size,position,stride", N.RINGS)
def test_n_step_one_returns_the_sampled_rows(capacity, size, position, stride):
    ring, cut = N.random_ring(capacity, N.RING_SEED + capacity)
    idx = N.given_idx(capacity, size, position, stride, 1, 257)
    staged, steps = N.rows(ring, cut, size, position, stride, 1, 0.99, idx)
    assert (steps == 1).all()
    assert np.array_equal(staged.view(np.uint32), ring[idx].view(np.uint32))


def test_kernel_cases_cover_every_horizon_and_cause():
    """What tests/test_gpu_nstep.py runs on the device, counted on the host: every horizon
    1 .. NAV_NSTEP_MAX and each of the four ending causes occurs; rewards of +-50 and of both
    signs are summed; the stride == capacity ring has horizon 1 only."""
    hor, why = collections.Counter(), collections.Counter()
    for capacity, size, position, stride in N.RINGS:
        ring, cut = N.random_ring(capacity, N.RING_SEED + capacity)
        assert 0.1 < cut.mean() < 0.3 and 0.01 < (ring[:, 7] != 0).mean() < 0.1
        assert (cut[ring[:, 7] != 0] == 1).all()
        assert (ring[:, 4] == 50).any() and (ring[:, 4] == -50).any()
        for n_step in N.NSTEPS:
            for B in N.BATCHES:
                for idx in (N.given_idx(capacity, size, position, stride, n_step, B),
                            N.draw(size, B, SEED, 5)):
                    c = []
                    _, steps = N.rows(ring, cut, size, position, stride, n_step, 0.99, idx, c)
                    hor.update(steps.tolist())
                    why.update(c)
                    assert stride < capacity or (steps == 1).all()
    assert set(hor) == set(range(1, N.NSTEP_MAX + 1)), sorted(hor)
    assert set(why) == set(N.CAUSES), why


def test_draw_is_the_row_kernels_draw():
    """(w.x * size) >> 32: within [0, size), the same for the same counter, another stream for
    another counter."""
    a = N.draw(1000, 300, SEED, 3)
    assert a.min() >= 0 and a.max() < 1000 and len(set(a.tolist())) > 200
    assert np.array_equal(a, N.draw(1000, 300, SEED, 3))
    assert not np.array_equal(a, N.draw(1000, 300, SEED, 4))
    assert np.array_equal(N.draw(1, 10, SEED, 3), np.zeros(10, np.int64))


def test_stamp_takes_bit_three_and_wraps():
    cut = np.full(10, 7, np.uint8)
    flags = np.array([0x08, 0x07, 0x1F, 0x10, 0x09], np.uint8)
    got = N.stamp(cut, 8, flags)
    assert got.tolist() == [1, 0, 1, 7, 7, 7, 7, 7, 1, 0]
    assert np.array_equal(N.stamp(cut, 3, flags[:0]), cut)


# ---- host validation of the two entry points
@pytest.fixture(scope="module")
def raw():
    return load_raw()


@pytest.mark.parametrize("fn,what,changed", BAD, ids=[f"{b[0]}-{b[1]}" for b in BAD])
def test_bad_arguments_return_einval(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == EINVAL


def test_every_listed_entry_point_has_a_case():
    assert {b[0] for b in BAD} == set(CALLS)


def test_empty_stamp_needs_no_device(raw):
    assert CALLS["nav_nstep_stamp"](raw, n=_v(0)) == 0


def test_header_and_package_agree_on_the_longest_horizon():
    import os
    import re
    from conftest import ROOT
    from nav import config as K
    src = open(os.path.join(ROOT, "include", "navenv.h")).read()
    (n,) = re.findall(r"#define NAV_NSTEP_MAX (\d+)", src)
    assert int(n) == K.NSTEP_MAX == N.NSTEP_MAX


# ---- refusals that need no device
def test_config_default_is_off_and_checks_its_range():
    from nav import config as K
    assert K.TD3Config().n_step == 1
    K.TD3Config().check_n_step()
    K.TD3Config(n_step=K.NSTEP_MAX).check_n_step()
    for bad in (0, -1, K.NSTEP_MAX + 1, 2.0, None):
        with pytest.raises(ValueError, match="n_step"):
            K.TD3Config(n_step=bad).check_n_step()


class _Hook:
    world_size = 1

    def __call__(self, bucket):
        return None


@pytest.mark.parametrize("kw", [dict(demo_fraction=0.25), dict(bc_weight=1.0),
                                dict(demo_fraction=0.25, bc_weight=1.0)],
                         ids=["demo_fraction", "bc_weight", "both"])
def test_learner_refuses_before_it_allocates(kw):
    from nav import config as K
    from nav.td3 import TD3
    with pytest.raises(ValueError, match="multi-step returns"):
        TD3(K.TD3Config(n_step=3, **kw), device="cuda")
    with pytest.raises(ValueError, match="multi-step returns"):
        TD3(K.TD3Config(n_step=3), device="cuda", grad_hook=_Hook())
    with pytest.raises(ValueError, match="n_step"):
        TD3(K.TD3Config(n_step=17), device="cuda")


@pytest.mark.parametrize("kw", [dict(demo_fraction=0.25), dict(bc_weight=1.0),
                                dict(grad_hook=_Hook()), dict(overlap_collect=True)],
                         ids=["demo_fraction", "bc_weight", "grad_hook", "overlap_collect"])
def test_trainer_refuses_before_it_builds(kw):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="multi-step returns"):
        VecTrainer(n_envs=256, hidden=64, batch=128, n_step=3, **kw)
    with pytest.raises(ValueError, match="n_step"):
        VecTrainer(n_envs=256, hidden=64, batch=128, n_step=0)


def test_population_refuses_an_n_step_member():
    from nav.population import PopulationTrainer
    with pytest.raises(ValueError, match="multi-step returns"):
        PopulationTrainer([{}, {"n_step": 3}], envs_per_member=64, hidden=64, batch=64,
                          envs_per_group=64, demos=False)
