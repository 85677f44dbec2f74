"""Resets to demonstration states on the GPU: nav_demo_reset against the host restatement
tests/demo_reset_ref.py bit for bit (the state, the counts, and nothing else of the SoA), every
tick form issuing it (a lockstep twin without the feature, passed through the restatement), off
means off, determinism and checkpoint resume, and a population's per-member probabilities through
an exploit. Everything compared is exact: the kernel copies an f32 state into an f64 one and
counts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import demo_reset_ref as D
import mlp_ref as R
from gpu_support import nav  # noqa: F401
from pop_support import same as _same, snapshot

pytestmark = pytest.mark.gpu
DEV = R.DEV
SEED = 1707366464
SLO, SHI = SEED & 0xFFFFFFFF, SEED >> 32
SOA = ("state", "goal", "region", "hist", "meta", "plan_index", "path_length", "episodes",
       "noise_scale")


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---------------------------------------------------------------- the kernel
N_ENVS, EPG, N_DEMOS, T = 200, 64, 3, 7   # a ragged last 64-row and block; the last group: 8 envs
USABLE = np.array([1, 6, 3, 2, 6, 1, 5, 4, 1, 6, 2, 3], np.int32)  # [4 groups * 3], 1 and T - 1


@pytest.fixture(scope="module")
def case():
    """The seeded inputs of the kernel test on the host, built once and left unchanged."""
    rng = np.random.default_rng(9)
    n = N_ENVS
    soa = {"state": rng.random((n, 2)) * 100, "goal": rng.random((n, 2)) * 100,
           "region": rng.random((n, 4)) * 100, "hist": rng.random((5, n, 2)) * 100,
           "meta": rng.integers(0, 1 << 15, n).astype(np.int32),
           "plan_index": rng.integers(0, 50, n).astype(np.int32),
           "path_length": rng.integers(50, 500, n).astype(np.int32),
           # episode numbers small and above 2^16
           "episodes": np.where(rng.random(n) < 0.5, rng.integers(5, 100, n),
                                rng.integers(1 << 16, 1 << 30, n)).astype(np.int32),
           "noise_scale": rng.random(n)}
    # bit 3 on about half, every other bit free
    flags = (rng.integers(0, 256, n) & 0xF7 | np.where(rng.random(n) < 0.5, 8, 0)).astype(np.uint8)
    demo = (rng.random((4 * N_DEMOS, T, 2)) * 100).astype(np.float32)
    assert (soa["episodes"] > 1 << 16).any() and 60 < ((flags & 8) != 0).sum() < 140
    assert ((flags & 8) != 0)[192:].any()  # the ragged row has reset envs
    return dict(soa=soa, flags=flags, demo=demo)


def launch(case, prob, prob_group=None, times=1, counts=True):
    """nav_demo_reset `times` times on device copies -> (the SoA after, counts or None)."""
    from nav._lib import NavEnvSoa, lib, ptr, stream_handle
    dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in case["soa"].items()}
    soa = NavEnvSoa(N_ENVS, *[dev[k].data_ptr() for k in SOA])
    flags = torch.from_numpy(case["flags"]).to(DEV)
    demo = torch.from_numpy(case["demo"]).to(DEV)
    us = torch.from_numpy(USABLE).to(DEV)
    pg = None if prob_group is None else torch.tensor(prob_group, dtype=torch.float64, device=DEV)
    cnt = torch.zeros((N_ENVS + 63) // 64, dtype=torch.int64, device=DEV) if counts else None
    for _ in range(times):
        lib().nav_demo_reset(C.byref(soa), ptr(flags), SLO, SHI, ptr(demo), ptr(us), N_DEMOS, T,
                             EPG, prob, ptr(pg), ptr(cnt), stream_handle())
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy(), case["flags"])
    assert np.array_equal(demo.cpu().numpy().view(np.uint32), case["demo"].view(np.uint32))
    return {k: v.cpu().numpy() for k, v in dev.items()}, None if cnt is None else cnt.cpu().numpy()


FORMS = [(0.25, None), (1.0, None), (0.0, (0.0, 1.0, 0.5, 0.25))]


@pytest.mark.parametrize("prob,prob_group", FORMS, ids=["p0.25", "p1", "per_group"])
def test_kernel_follows_the_restatement(nav, case, prob, prob_group):
    soa, flags = case["soa"], case["flags"]
    want, want_counts, picks = D.reset(soa["state"], flags, soa["episodes"], SEED, case["demo"],
                                       USABLE, N_DEMOS, EPG, prob, prob_group)
    took = picks[:, 0] >= 0
    print(f"reset envs {int(((flags & 8) != 0).sum())}, took {int(took.sum())}, "
          f"counts {want_counts.tolist()}")
    assert 0 < took.sum() and (~took).any()
    got, counts = launch(case, prob, prob_group)
    assert np.array_equal(bits64(got["state"]), bits64(want))
    for k in SOA[1:]:  # nothing else of the SoA is written
        assert got[k].tobytes() == soa[k].tobytes(), k
    assert np.array_equal(counts, want_counts) and counts.sum() == took.sum()
    # envs without bit 3 keep their state; the counts are cumulative
    assert np.array_equal(bits64(got["state"][~took]), bits64(soa["state"][~took]))
    again, twice = launch(case, prob, prob_group, times=2)
    assert np.array_equal(twice, 2 * want_counts)
    assert np.array_equal(bits64(again["state"]), bits64(want))
    # counts is optional
    none, c = launch(case, prob, prob_group, counts=False)
    assert c is None and np.array_equal(bits64(none["state"]), bits64(want))


def test_at_probability_one_every_reset_env_sits_on_its_groups_demonstrations(nav, case):
    got, counts = launch(case, 1.0)
    reset = (case["flags"] & 8) != 0
    assert counts.sum() == reset.sum()
    demo = case["demo"].astype(np.float64)
    cells = set()
    for e in np.flatnonzero(reset):
        g = e // EPG
        allowed = [(d, t) for d in range(N_DEMOS) for t in range(USABLE[g * N_DEMOS + d])]
        hit = [c for c in allowed if np.array_equal(demo[g * N_DEMOS + c[0], c[1]],
                                                    got["state"][e])]
        assert len(hit) == 1, e
        cells.add((g, *hit[0]))
    assert len(cells) > 20  # spread over the groups' usable cells, not one favourite


def test_bad_arguments_launch_nothing(nav, case):
    """The host-side refusals of tests/test_demo_reset_cpu.py on live buffers."""
    from nav._lib import NavEnvSoa, lib
    dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in case["soa"].items()}
    soa = NavEnvSoa(N_ENVS, *[dev[k].data_ptr() for k in SOA])
    flags = torch.full((N_ENVS,), 8, dtype=torch.uint8, device=DEV)
    demo = torch.from_numpy(case["demo"]).to(DEV)
    us = torch.from_numpy(USABLE).to(DEV)
    cnt = torch.zeros(4, dtype=torch.int64, device=DEV)
    ok = [C.byref(soa), flags.data_ptr(), SLO, SHI, demo.data_ptr(), us.data_ptr(), N_DEMOS, T,
          EPG, 1.0, None, cnt.data_ptr(), None]
    for pos, bad in ((1, None), (4, None), (5, None), (6, 0), (7, 1), (8, 0), (9, 1.5),
                     (9, float("nan")), (9, -1.0)):
        args = list(ok)
        args[pos] = bad
        assert lib().raw.nav_demo_reset(*args) == -100000, (pos, bad)
    torch.cuda.synchronize()
    assert (cnt == 0).all()
    assert np.array_equal(bits64(dev["state"].cpu().numpy()), bits64(case["soa"]["state"]))


# ---------------------------------------------------------------- the ticks
TRAINER = dict(n_envs=256, hidden=64, batch=128, replay_capacity=1024, envs_per_group=64)
PROB = 0.5


def quick_episodes(env):
    """Paths that end within 8 ticks, staggered: env e's path ends at tick 1 + e % 8, paths of 3
    steps among them. The tick's done test is plan_index == path_length - 1 and nav_env_init
    leaves plan_index at 5, which a path_length0 of 3 would never meet, so the two counters are
    set here instead of through path_length0."""
    e = torch.arange(env.n, dtype=torch.int32, device=env.device)
    env.plan_index.fill_(1)
    env.path_length.copy_(2 + e % 8)


def cem_usable(tr):
    """(the CEM's states on the host, the restatement's usable table) of a trainer."""
    st, _, goals = tr._cem
    st = st.cpu().numpy()
    return st, D.usable(st, goals, 5.0)


def twin_tick(a, b, sync, tick):
    """One lockstep tick: the twin b (no feature) takes a copy of a's whole SoA, `sync` hands it
    the step and the ring position, both tick. -> a's and b's SoA and flags on the host."""
    for k in SOA:
        getattr(b.env, k).copy_(getattr(a.env, k))
    sync()
    tick(a)
    tick(b)
    torch.cuda.synchronize()
    host = lambda t: {k: getattr(t.env, k).cpu().numpy() for k in SOA + ("flags",)}  # noqa: E731
    return host(a), host(b)


def check_tick(ha, hb, demo, usable, prob, prob_group=None):
    """The feature env's state is the twin's passed through the restatement; the rest equal."""
    want, counts, picks = D.reset(hb["state"], hb["flags"], hb["episodes"], SEED, demo, usable, 3,
                                  64, prob, prob_group)
    assert np.array_equal(ha["flags"], hb["flags"])
    for k in SOA[1:]:
        assert ha[k].tobytes() == hb[k].tobytes(), k
    assert np.array_equal(bits64(ha["state"]), bits64(want))
    return int(((hb["flags"] & 8) != 0).sum()), counts


@pytest.fixture(scope="module")
def pair(nav):
    """A trainer with the feature and its twin without (short paths: quick_episodes)."""
    from nav.trainer import VecTrainer
    return (VecTrainer(device=DEV, **TRAINER, demo_reset_prob=PROB),
            VecTrainer(device=DEV, **TRAINER))


@pytest.mark.parametrize("form", ["act_tick", "agent_step_fused", "agent_step_two_launch"])
def test_every_tick_form_issues_it(nav, pair, form):
    a, b = pair
    for t in (a, b):
        t.fuse_tick = form == "act_tick"
        t.env.fuse_demo = form != "agent_step_two_launch"
    quick_episodes(a.env)
    demo, usable = cem_usable(a)
    assert np.array_equal(a.env._dreset["usable"].cpu().numpy(), usable)
    assert usable.min() >= 1 and usable.max() <= demo.shape[1] - 1
    launches, total = a.env.demo_reset_launches, a.env.demo_resets.cpu().numpy().copy()

    def sync():
        b.steps = a.steps
        b.replay.position, b.replay.size = a.replay.position, a.replay.size
    ticks_with_resets = taken = 0
    for _ in range(8):
        ha, hb = twin_tick(a, b, sync, lambda t: t.collect())
        n_reset, counts = check_tick(ha, hb, demo, usable, PROB)
        ticks_with_resets += n_reset > 0
        taken += int(counts.sum())
        total += counts
    print(form, "ticks with resets", ticks_with_resets, "taken", taken)
    assert ticks_with_resets >= 6 and taken > 40
    assert a.env.demo_reset_launches == launches + 8 and b.env.demo_reset_launches == 0
    assert np.array_equal(a.env.demo_resets.cpu().numpy(), total)
    assert b.env.demo_resets is None
    assert torch.equal(a.replay.rows, b.replay.rows)  # the ticks pushed the same rows


POP = dict(envs_per_member=128, hidden=64, batch=128, envs_per_group=64, replay_capacity=1024)


@pytest.fixture(scope="module")
def pop_pair(nav):
    from nav.population import PopulationTrainer
    a = PopulationTrainer([{"demo_reset_prob": 0.25}, {"demo_reset_prob": 1.0}], device=DEV, **POP)
    b = PopulationTrainer([{}, {}], device=DEV, **POP)
    return a, b


def pop_sync(a, b):
    def sync():
        b.steps = a.steps
        for ra, rb in zip(a.rings, b.rings):
            rb.position, rb.size = ra.position, ra.size
    return sync


def test_the_population_tick_issues_it_per_member(nav, pop_pair):
    a, b = pop_pair
    quick_episodes(a.env)
    demo, usable = cem_usable(a)
    assert a.env._dreset["prob_group"].tolist() == [0.25, 0.25, 1.0, 1.0]
    assert a.env._dreset["prob"] == 0.0
    per_member = np.zeros(2, np.int64)
    resets = np.zeros(2, np.int64)
    for _ in range(8):
        ha, hb = twin_tick(a, b, pop_sync(a, b), lambda t: t.collect())
        _, counts = check_tick(ha, hb, demo, usable, 0.0, (0.25, 0.25, 1.0, 1.0))
        per_member += counts.reshape(2, 2).sum(1)
        resets += ((hb["flags"] & 8) != 0).reshape(2, 128).sum(1)
    print("resets", resets.tolist(), "taken", per_member.tolist())
    assert per_member[1] == resets[1] and 0 < per_member[0] < resets[0]
    assert a.env.demo_reset_launches == 8 and b.env.demo_resets is None
    assert np.array_equal(a.env.demo_resets.cpu().numpy().reshape(2, 2).sum(1), per_member)
    for m in range(2):
        share = per_member[m] / float(a.env.episodes[a.member_slice(m)].sum().item())
        assert a.demo_reset_share(m) == share


def test_exploit_hands_the_probability_to_the_clone(nav, pop_pair):
    """Member 0 (0.25) becomes a clone of member 1 (1.0): the value follows, the table is rebuilt,
    and the next tick uses it on the clone's groups."""
    a, b = pop_pair
    ev = a.exploit([1], [0])
    assert a.member_value(0, "demo_reset_prob") == 1.0 and a.members[0]["demo_reset_prob"] == 1.0
    assert ev[0]["before"]["demo_reset_prob"] == 0.25 and ev[0]["after"]["demo_reset_prob"] == 1.0
    assert a.env._dreset["prob_group"].tolist() == [1.0, 1.0, 1.0, 1.0]
    b.exploit([1], [0])  # the twin's learners follow (its ticks read member 0's actor)
    before = a.env.demo_resets.cpu().numpy().copy()
    quick_episodes(a.env)
    a.env.path_length.fill_(2)  # every env's path ends on this tick
    demo, usable = cem_usable(a)
    ha, hb = twin_tick(a, b, pop_sync(a, b), lambda t: t.collect())
    n_reset, counts = check_tick(ha, hb, demo, usable, 0.0, (1.0, 1.0, 1.0, 1.0))
    assert n_reset == 256 and counts.sum() == 256
    assert np.array_equal(a.env.demo_resets.cpu().numpy(), before + counts)
    # an explored value lands in the table too
    a.exploit([1], [0], explore={"demo_reset_prob": (0.0, 0.9)})
    assert a.member_value(0, "demo_reset_prob") in (0.8, 0.9)
    assert a.env._dreset["prob_group"].tolist()[:2] == [a.member_value(0, "demo_reset_prob")] * 2


# ---------------------------------------------------------------- the trainer
def _snapshot(tr):
    return snapshot(tr, "env")


def test_off_means_off(nav):
    from nav.trainer import VecTrainer
    snaps = []
    for kw in (dict(demo_reset_prob=0), {}):
        tr = VecTrainer(device=DEV, **TRAINER, **kw)
        quick_episodes(tr.env)
        for _ in range(12):
            tr.step()
        torch.cuda.synchronize()
        assert tr.env.demo_reset_launches == 0 and tr.env.demo_resets is None
        assert tr.env._dreset is None and tr.env.demo_reset_share() == 0.0
        assert int(tr.env.episodes.sum()) > 5 * 256  # episodes did end
        assert "demo_reset" not in tr.state_dict()
        snaps.append(_snapshot(tr))
    assert len(snaps[0]) == 6 + 1 + len(SOA) and _same(*snaps)
    assert snaps[0]["actor"].abs().max() > 0


def test_determinism_and_resume(nav, tmp_path):
    from nav.trainer import VecTrainer
    a, b = (VecTrainer(device=DEV, **TRAINER, demo_reset_prob=0.3) for _ in range(2))
    for t in (a, b):
        quick_episodes(t.env)
    for _ in range(20):
        a.step()
    for _ in range(10):
        b.step()
    path = os.path.join(tmp_path, "demo_reset.pt")
    b.save(path)
    c = VecTrainer.load(path, device=DEV)
    assert c.demo_reset_prob == 0.3 and c.env._dreset["prob"] == 0.3
    assert torch.equal(c.env.demo_resets, b.env.demo_resets)
    assert torch.equal(c.env._dreset["usable"], b.env._dreset["usable"])
    assert torch.equal(c.env._dreset["states"], b.env._dreset["states"])
    for _ in range(10):
        b.step()
        c.step()
    torch.cuda.synchronize()
    taken = int(a.env.demo_resets.sum())
    print("taken", taken, "share", a.env.demo_reset_share())
    assert taken > 20
    assert _same(_snapshot(a), _snapshot(b)) and _same(_snapshot(a), _snapshot(c))
    assert torch.equal(a.env.demo_resets, b.env.demo_resets)
    assert torch.equal(a.env.demo_resets, c.env.demo_resets)
    assert a.env.demo_reset_share() == b.env.demo_reset_share() == c.env.demo_reset_share() > 0
    assert a.env.demo_reset_share() == taken / float(a.env.episodes.sum())
    assert a.env.demo_reset_launches == 20 and c.env.demo_reset_launches == 10
    # a checkpoint written with the feature off loads with it off
    plain = VecTrainer(device=DEV, **TRAINER)
    plain.step()
    off = VecTrainer.from_state_dict(plain.state_dict(), device=DEV)
    assert off.demo_reset_prob == 0.0 and off.env._dreset is None and off.env.demo_resets is None
