"""Prioritised replay, host side: every argument set below is refused by the nav_per_* entry
points and nav_td3_critic_rows_w with the raw status NAV_EINVAL before any HIP call (no kernel is
launched, the dummy pointers are never followed, so no GPU is needed), and the host restatement
(tests/per_ref.py) agrees with itself: its sampler with numpy's searchsorted on the cumulative
sums, its draw frequencies with the priorities' shares, its update with the duplicate rule."""
import ctypes as C

import numpy as np
import pytest

import per_ref as P
from abi_args import EINVAL, F, Call, load_raw
from abi_args import v as _v

NAN = float("nan")
SEED = 1707366464


@pytest.fixture(scope="module")
def raw():
    return load_raw()


def per(pri=F, sums=F, stat=F, capacity=1000):
    from nav._lib import NavPer
    return lambda: C.byref(NavPer(pri, sums, stat, capacity))


def net(d_in=4, d_out=1):
    from nav._lib import NavMlp
    return NavMlp(d_in, d_out, 64, 64, 2, F, F)


def nets(*ns):
    from nav._lib import NavMlp
    return (NavMlp * len(ns))(*ns)


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def replay():
    from nav._lib import NavReplay
    return C.byref(NavReplay(F, 1000))


PAIR = lambda: ptrs(F, F)  # noqa: E731
TWINS = lambda: nets(net(), net())  # noqa: E731

CALLS = {c.fn: c for c in (
    Call("nav_per_sums_count", capacity=_v(1000)),
    Call("nav_per_init", per=per(), stream=_v(None)),
    Call("nav_per_stamp", per=per(), pos=_v(10), n=_v(100), stream=_v(None)),
    Call("nav_per_sums", per=per(), size=_v(500), stream=_v(None)),
    Call("nav_per_sample", per=per(), size=_v(500), B=_v(64), seed_lo=_v(1), seed_hi=_v(2),
         counter=_v(3), beta=_v(0.4), idx_critic=_v(F), w_critic=_v(F), idx_actor=_v(F),
         stream=_v(None)),
    Call("nav_per_update", per=per(), B=_v(64), idx=_v(F), td1=_v(F), td2=_v(F), alpha=_v(0.6),
         eps=_v(1e-6), stream=_v(None)),
    Call("nav_td3_critic_rows_w", target_actor=lambda: C.byref(net(2, 2)), target_critics=TWINS,
         critics=TWINS, replay=replay, size=_v(500), B=_v(64), idx=_v(None), seed_lo=_v(1),
         seed_hi=_v(2), counter=_v(3), eps=_v(None), policy_noise=_v(0.2), noise_clip=_v(0.5),
         max_action=_v(5.0), gamma=_v(0.99), batch=_v(F), dq=PAIR, loss_part=PAIR,
         edge_slabs=PAIR, acts=_v(None), save_mask=_v(0), masks=PAIR, row_backward=_v(1),
         dz=_v(None), dz_save_mask=_v(0), split_twins=_v(-1), w=_v(F), td_abs=PAIR,
         stream=_v(None)),
)}

PER_FNS = ("nav_per_init", "nav_per_stamp", "nav_per_sums", "nav_per_sample", "nav_per_update")

# (entry point, what is wrong, the altered arguments)
BAD = [("nav_per_sums_count", "capacity = 0", dict(capacity=_v(0))),
       ("nav_per_sums_count", "capacity = -5", dict(capacity=_v(-5)))]
BAD += [case for fn in PER_FNS for case in (
    (fn, "NULL struct", dict(per=_v(None))),
    (fn, "NULL pri", dict(per=per(pri=None))),
    (fn, "NULL sums", dict(per=per(sums=None))),
    (fn, "NULL stat", dict(per=per(stat=None))),
    (fn, "capacity = 0", dict(per=per(capacity=0))),
    (fn, "capacity < 0", dict(per=per(capacity=-1))),
)]
BAD += [case for fn in ("nav_per_sums", "nav_per_sample") for case in (
    (fn, "size = 0", dict(size=_v(0))),
    (fn, "size < 0", dict(size=_v(-3))),
    (fn, "size > capacity", dict(size=_v(1001))),
)]
BAD += [
    ("nav_per_stamp", "n < 0", dict(n=_v(-1))),
    ("nav_per_stamp", "n > capacity", dict(n=_v(1001))),
    ("nav_per_stamp", "pos < 0", dict(pos=_v(-1))),
    ("nav_per_stamp", "pos = capacity", dict(pos=_v(1000))),
    ("nav_per_stamp", "pos out of range, n = 0", dict(pos=_v(1000), n=_v(0))),
    ("nav_per_sample", "B = 0", dict(B=_v(0))),
    ("nav_per_sample", "B < 0", dict(B=_v(-64))),
    ("nav_per_sample", "beta < 0", dict(beta=_v(-0.1))),
    ("nav_per_sample", "beta NaN", dict(beta=_v(NAN))),
    ("nav_per_sample", "w_critic without idx_critic", dict(idx_critic=_v(None))),
    ("nav_per_update", "B = 0", dict(B=_v(0))),
    ("nav_per_update", "B < 0", dict(B=_v(-1))),
    ("nav_per_update", "no idx", dict(idx=_v(None))),
    ("nav_per_update", "no td1", dict(td1=_v(None))),
    ("nav_per_update", "no td2", dict(td2=_v(None))),
    ("nav_per_update", "alpha = 0", dict(alpha=_v(0.0))),
    ("nav_per_update", "alpha < 0", dict(alpha=_v(-0.6))),
    ("nav_per_update", "alpha NaN", dict(alpha=_v(NAN))),
    ("nav_per_update", "eps < 0", dict(eps=_v(-1e-6))),
    ("nav_per_update", "eps NaN", dict(eps=_v(NAN))),
    ("nav_td3_critic_rows_w", "no w", dict(w=_v(None))),
    ("nav_td3_critic_rows_w", "no td_abs", dict(td_abs=_v(None))),
    ("nav_td3_critic_rows_w", "td_abs[0] NULL", dict(td_abs=lambda: ptrs(None, F))),
    ("nav_td3_critic_rows_w", "td_abs[1] NULL", dict(td_abs=lambda: ptrs(F, None))),
    # what nav_td3_critic_rows refuses, the weighted form refuses too
    ("nav_td3_critic_rows_w", "B = 0", dict(B=_v(0))),
    ("nav_td3_critic_rows_w", "no batch", dict(batch=_v(None))),
    ("nav_td3_critic_rows_w", "size = 0", dict(size=_v(0))),
]


@pytest.mark.parametrize("fn,what,changed", BAD, ids=[f"{b[0]}-{b[1]}" for b in BAD])
def test_bad_arguments_return_einval(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == EINVAL


def test_every_listed_entry_point_has_a_case():
    assert {b[0] for b in BAD} == set(CALLS)


def test_no_op_calls_need_no_device(raw):
    """n = 0 stamps nothing and a sample with no output array draws nothing: both return 0
    without a launch; the workspace size is a pure function of the capacity and grows with it."""
    assert CALLS["nav_per_stamp"](raw, n=_v(0)) == 0
    assert CALLS["nav_per_sample"](raw, idx_critic=_v(None), w_critic=_v(None),
                                   idx_actor=_v(None)) == 0
    counts = [raw.nav_per_sums_count(c) for c in (1, 1024, 1025, 262144, (1 << 20) + 37)]
    assert all(c > 0 for c in counts) and counts == sorted(counts)
    # at least one u64 per 32 rows, one per 1 024 rows and the total
    assert counts[3] >= 262144 // 32 + 262144 // 1024 + 1


# ---- the restatement against itself
@pytest.mark.parametrize("size,B,hi", [(1, 50, 1 << 31), (37, 500, 1 << 31), (5000, 2000, 1 << 31),
                                       (300, 2000, 4)])
def test_sample_equals_searchsorted(size, B, hi):
    rng = np.random.default_rng(size)
    pri = rng.integers(1, hi, size + 20, dtype=np.int64)
    pri[size:] = 0xFFFFFFFF  # beyond size: never read
    for actor in (False, True):
        got = P.sample(pri, size, B, SEED, 11, actor)
        cum = np.cumsum(pri[:size].astype(np.uint64))
        t = np.array(P.targets(int(cum[-1]), B, SEED, 11, actor), np.uint64)
        assert np.array_equal(got, np.searchsorted(cum, t, side="right"))
        assert got.min() >= 0 and got.max() < size
    assert not np.array_equal(P.sample(pri, size, B, SEED, 11, False),
                              P.sample(pri, size, B, SEED, 11, True)) or size == 1


def test_zero_priority_rows_are_never_drawn():
    pri = np.array([0, 5, 0, 0, 7, 0], np.int64)
    got = P.sample(pri, 6, 3000, SEED, 2, False)
    assert set(got.tolist()) == {1, 4}


def test_draw_frequencies_follow_the_priorities():
    """8 rows of 1, 2, 4, ..., 128 counts, 200 000 draws: every row's count within 5 binomial
    standard deviations of B p_k / S."""
    B = 200_000
    pri = np.array([1 << k for k in range(8)], np.int64)
    S = int(pri.sum())
    counts = np.bincount(P.sample(pri, 8, B, SEED, 5, False), minlength=8)
    for k in range(8):
        p = int(pri[k]) / S
        sd = np.sqrt(B * p * (1 - p))
        print(f"row {k}: {counts[k]} draws, expected {B * p:.1f} +- {sd:.1f}")
        assert abs(counts[k] - B * p) <= 5 * sd, k


def test_update_keeps_the_maximum_and_discards_the_old_value():
    pri = np.array([900, 900, 900, 900, 900], np.int64)
    idx = np.array([1, 3, 1, 1, 3, 4])
    q = np.array([7, 50, 9, 8, 20, 1])
    got = P.update(pri, idx, q)
    assert got.tolist() == [900, 9, 900, 50, 1]  # not max(900, .): the old value goes


def test_priority_formula_and_clamps():
    td1 = np.array([0.0, 1e-30, 1.0, 1e4, np.inf, np.nan, -3.0], np.float32)
    td2 = np.array([0.0, 0.0, 1.0, 1e4, 1.0, 1.0, 3.0], np.float32)
    q = P.priority(td1, td2, 0.6, 1e-6)
    a, e = float(np.float32(0.6)), float(np.float32(1e-6))
    assert q[0] == int(np.floor(e ** a * 65536 + 0.5)) and q[0] >= 1
    assert q[2] == int(np.floor((1.0 + e) ** a * 65536 + 0.5))
    assert q[4] == P.MAX_PRI and q[5] == 1
    assert q[6] == int(np.floor((3.0 + e) ** a * 65536 + 0.5))
    # alpha = 2 on zeros underflows to 0 counts: stored as 1; 1e4^2 clamps at 2^31 - 1
    q2 = P.priority(td1[:4], td2[:4], 2.0, 0.0)
    assert q2.tolist() == [1, 1, 65536, P.MAX_PRI]


def test_weights_are_one_for_equal_priorities_and_at_most_one():
    pri = np.full(40, 12345, np.int64)
    assert (P.weights(pri, 40, np.arange(40), 0.7) == np.float32(1.0)).all()
    pri = np.arange(1, 41, dtype=np.int64) * 1000
    w = P.weights(pri, 40, np.arange(40), 0.4)
    assert w[0] == np.float32(1.0) and (w <= 1).all() and (w > 0).all()
    assert np.all(np.diff(w) <= 0)
