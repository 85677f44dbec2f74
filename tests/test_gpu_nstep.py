"""Multi-step returns on the GPU: nav_nstep_rows and nav_nstep_stamp against the host restatement
tests/nstep_ref.py bit for bit, the ticks' cut marks against their flags, the critic launch on the
staged rows against the plain launch and an fp64 n-step target, and the trainer's plumbing (off
means off, horizon one is the plain epoch, epochs follow the restatement with and without
prioritised replay, checkpoints, the rejected combinations).

Everything the gather writes is exact: the host restatement uses the same double and f32
operations. The only bound is the project's own for a split-GEMM result against fp64
(test_gpu_mlp.py: 2e-6 of scale), on the critic's target."""
import collections
import ctypes as C
import os

import numpy as np
import pytest
import torch

import launches as LN
import mlp_ref as R
import nstep_ref as N
import per_ref as P
from gpu_support import nav  # noqa: F401
from nstep_args import BAD, CALLS
from pop_support import moments as _moments, params as _params, same as _same, snapshot

pytestmark = pytest.mark.gpu
DEV = R.DEV
SEED, SLO, SHI = LN.SEED, LN.SLO, LN.SHI
GAMMA = 0.99
COUNTER = 5


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---------------------------------------------------------------- the kernels
_RINGS = {}


def ring_case(capacity):
    """The seeded ring of a capacity on the host and the device, built once."""
    if capacity not in _RINGS:
        from nav._lib import NavReplay
        ring, cut = N.random_ring(capacity, N.RING_SEED + capacity)
        d = dict(ring=ring, cut=cut, rows=torch.from_numpy(ring).to(DEV),
                 dcut=torch.from_numpy(cut).to(DEV))
        d["rd"] = NavReplay(d["rows"].data_ptr(), capacity)
        _RINGS[capacity] = d
    return _RINGS[capacity]


def gather(case, size, position, stride, n_step, B, idx=None, counter=COUNTER, steps=True,
           gamma=GAMMA):
    """nav_nstep_rows into NaN / -1 filled outputs -> (staged [B][8], steps [B] or None)."""
    from nav._lib import lib, ptr, stream_handle
    staged = torch.full((B, 8), float("nan"), device=DEV)
    st = torch.full((B,), -1, dtype=torch.int32, device=DEV) if steps else None
    di = None if idx is None else torch.from_numpy(np.asarray(idx, np.int64)).to(DEV)
    lib().nav_nstep_rows(C.byref(case["rd"]), ptr(case["dcut"]), size, position, stride, n_step,
                         gamma, B, ptr(di), SLO, SHI, counter, ptr(staged), ptr(st),
                         stream_handle())
    torch.cuda.synchronize()
    return staged.cpu().numpy(), None if st is None else st.cpu().numpy()


@pytest.mark.parametrize("n_step", N.NSTEPS)
@pytest.mark.parametrize("capacity,size,position,stride", N.RINGS,
                         ids=["-".join(map(str, r)) for r in N.RINGS])
def test_rows_follow_the_restatement(nav, capacity, size, position, stride, n_step):
    from nav._lib import lib, ptr, stream_handle
    case = ring_case(capacity)
    for B in N.BATCHES:
        given = N.given_idx(capacity, size, position, stride, n_step, B)
        drawn = N.draw(size, B, SEED, COUNTER)
        for idx, passed in ((given, given), (drawn, None)):
            got, steps = gather(case, size, position, stride, n_step, B, passed)
            want, want_steps = N.rows(case["ring"], case["cut"], size, position, stride, n_step,
                                      GAMMA, idx)
            assert np.array_equal(steps, want_steps), (B, passed is None)
            assert np.array_equal(bits(got), bits(want)), (B, passed is None)
            assert np.array_equal(got[:, 0], idx)  # column 0 of the seeded ring: the row index
            one = steps == 1
            assert np.array_equal(bits(got[one]), bits(case["ring"][idx[one]]))
        # idx NULL: the rows nav_replay_sample draws at the same 2*counter
        batch = torch.full((B, 8), float("nan"), device=DEV)
        lib().nav_replay_sample(C.byref(case["rd"]), size, B, None, SLO, SHI, 2 * COUNTER,
                                ptr(batch), stream_handle())
        torch.cuda.synchronize()
        assert np.array_equal(batch.cpu().numpy()[:, 0], drawn)
        assert np.array_equal(bits(batch.cpu().numpy()[:, :4]), bits(got[:, :4]))
    # the ring and the marks are read only
    assert np.array_equal(bits(case["rows"].cpu().numpy()), bits(case["ring"]))
    assert np.array_equal(case["dcut"].cpu().numpy(), case["cut"])


def test_cases_cover_every_horizon_and_cause():
    """Under the restatement the parametrised set above reaches every horizon 1 .. NAV_NSTEP_MAX
    and each of the four ending causes: no degenerate input passes silently."""
    hor, why = collections.Counter(), collections.Counter()
    for capacity, size, position, stride in N.RINGS:
        case = ring_case(capacity)
        for n_step in N.NSTEPS:
            for B in N.BATCHES:
                for idx in (N.given_idx(capacity, size, position, stride, n_step, B),
                            N.draw(size, B, SEED, COUNTER)):
                    c = []
                    _, steps = N.rows(case["ring"], case["cut"], size, position, stride, n_step,
                                      GAMMA, idx, c)
                    hor.update(steps.tolist())
                    why.update(c)
    print(sorted(hor.items()), dict(why))
    assert set(hor) == set(range(1, N.NSTEP_MAX + 1)) and set(why) == set(N.CAUSES)


def test_steps_is_optional_and_other_counters_draw_other_rows(nav):
    case = ring_case(4096)
    a, steps = gather(case, 4096, 1000, 64, 3, 257)
    b, none = gather(case, 4096, 1000, 64, 3, 257, steps=False)
    assert none is None and np.array_equal(bits(a), bits(b)) and steps.max() > 1
    c, _ = gather(case, 4096, 1000, 64, 3, 257, counter=COUNTER + 1)
    assert not np.array_equal(a[:, 0], c[:, 0])
    # gamma = 0 and 1 are allowed: R is the first reward / the plain sum
    idx = N.given_idx(4096, 4096, 1000, 64, 3, 257)
    for g in (0.0, 1.0):
        got, st = gather(case, 4096, 1000, 64, 3, 257, idx, gamma=g)
        want, wst = N.rows(case["ring"], case["cut"], 4096, 1000, 64, 3, g, idx)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(st, wst)


def test_stamp_follows_the_restatement(nav):
    from nav._lib import lib, ptr, stream_handle
    L, s = lib(), stream_handle()
    cap = 3000
    rng = np.random.default_rng(3)
    host = rng.integers(0, 2, cap).astype(np.uint8)
    cut = torch.from_numpy(host.copy()).to(DEV)
    # a range that wraps through slot 0; flags with every bit pattern around bit 3
    flags = rng.integers(0, 32, 250).astype(np.uint8)
    L.nav_nstep_stamp(ptr(cut), cap, 2900, 250, ptr(torch.from_numpy(flags).to(DEV)), s)
    want = N.stamp(host, 2900, flags)
    assert np.array_equal(cut.cpu().numpy(), want)
    assert np.array_equal(want[150:2900], host[150:2900])  # outside the range: unchanged
    assert set(want[2900:].tolist()) == {0, 1}
    L.nav_nstep_stamp(ptr(cut), cap, 17, 0, ptr(torch.from_numpy(flags).to(DEV)), s)  # n = 0
    assert np.array_equal(cut.cpu().numpy(), want)
    full = rng.integers(0, 32, cap).astype(np.uint8)  # n = capacity from the middle: every row
    L.nav_nstep_stamp(ptr(cut), cap, 1234, cap, ptr(torch.from_numpy(full).to(DEV)), s)
    assert np.array_equal(cut.cpu().numpy(), N.stamp(want, 1234, full))


@pytest.mark.parametrize("fn,what,changed", BAD, ids=[f"{b[0]}-{b[1]}" for b in BAD])
def test_bad_arguments_launch_nothing(nav, fn, what, changed):
    """The host-side refusals of tests/test_nstep_cpu.py on live buffers: NAV_EINVAL, and the
    outputs keep their fill."""
    from nav._lib import NavReplay, lib
    from abi_args import EINVAL, F
    from abi_args import v as _v
    rows = torch.zeros(1000, 8, device=DEV)
    cut = torch.full((1000,), 7, dtype=torch.uint8, device=DEV)
    flags = torch.full((1000,), 8, dtype=torch.uint8, device=DEV)
    staged = torch.full((64, 8), 5.0, device=DEV)
    live = {"cut": _v(cut.data_ptr()), "flags": _v(flags.data_ptr()),
            "staged": _v(staged.data_ptr()),
            "replay": lambda: C.byref(NavReplay(rows.data_ptr(), 1000))}
    args = {k: v for k, v in live.items() if k in CALLS[fn].valid}
    for k, v in changed.items():  # the case's own alteration wins; a dummy pointer stays one
        args[k] = v
    assert F == 16
    assert CALLS[fn](lib().raw, **args) == EINVAL
    torch.cuda.synchronize()
    assert (cut == 7).all() and (staged == 5.0).all()


# ---------------------------------------------------------------- the ticks
TRAINER = dict(n_envs=256, hidden=64, batch=128, replay_capacity=1024, envs_per_group=64)


@pytest.mark.parametrize("form", ["act_tick", "agent_step_fused", "agent_step_two_launch"])
def test_ticks_write_the_marks(nav, form):
    """80 ticks of 256 envs into a ring of 10 000 rows (no multiple of 256: the stamps wrap):
    every live row's mark is bit 3 of the flags of the tick that wrote it. Paths end at 50 steps
    (done), goals and stuck steps end an episode earlier (no done)."""
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, n_envs=256, hidden=64, batch=128, envs_per_group=64, n_step=3)
    if form != "act_tick":
        tr.fuse_tick = False
        tr.env.fuse_demo = form == "agent_step_fused"
    cap = tr.replay.capacity
    assert cap == 10000 and tr.replay.stride == 256 and tr.replay.cut.dtype == torch.uint8
    want = np.zeros(cap, np.uint8)
    seen = collections.Counter()
    for _ in range(80):
        base = tr.replay.position
        tr.collect()
        torch.cuda.synchronize()
        fl = tr.env.flags.cpu().numpy()
        want = N.stamp(want, base, fl)
        seen["ended"] += int(((fl >> 3) & 1).sum())
        seen["done"] += int((fl & 1).sum())
        seen["ended without done"] += int((((fl >> 3) & 1) & ~(fl & 1)).sum())
    print(form, dict(seen))
    assert len(tr.replay) == cap
    got = tr.replay.cut.cpu().numpy()
    assert np.array_equal(got, want)
    rows = tr.replay.rows.cpu().numpy()
    assert (got[rows[:, 7] != 0] == 1).all()  # a done row is a cut row
    assert seen["done"] > 0 and seen["ended without done"] > 0 and 0 < got.sum() < cap


# ---------------------------------------------------------------- the critic on staged rows
def _critic(nets, rd, idx, eps, B):
    """nav_td3_critic_rows on the ring descriptor `rd` of B rows into zeroed buffers."""
    return LN.critic_rows(nets, dict(idx=idx, eps=eps), B, fill=0.0, rd=rd, size=B, gamma=GAMMA)


@pytest.mark.parametrize("hidden", [64, 256])
def test_critic_sees_the_n_step_target(nav, hidden):
    from nav._lib import NavReplay, lib, ptr, stream_handle
    nh, B, n_step, stride, position = 2, 257, 3, 7, 123
    case = R.epoch_case(hidden, nh, B)
    nets, dev = LN.device_epoch(case)
    ring = case["rows"].numpy()
    rng = np.random.default_rng(11)
    cut = ((ring[:, 7] != 0) | (rng.random(R.RING) < 0.15)).astype(np.uint8)
    idx = case["idx"].numpy()
    dcut = torch.from_numpy(cut).to(DEV)
    rows, eps, didx = dev["rows"], dev["eps"], dev["idx"]
    # the device's staging, then the critic launch on the staged rows in order
    staged = torch.full((B, 8), float("nan"), device=DEV)
    steps = torch.zeros(B, dtype=torch.int32, device=DEV)
    lib().nav_nstep_rows(C.byref(NavReplay(rows.data_ptr(), R.RING)), ptr(dcut), R.RING, position,
                         stride, n_step, GAMMA, B, ptr(didx), SLO, SHI, 3, ptr(staged),
                         ptr(steps), stream_handle())
    iota = torch.arange(B, dtype=torch.int64, device=DEV)
    got = _critic(nets, NavReplay(staged.data_ptr(), B), iota, eps, B)
    # nav_td3_critic_rows directly on a ring whose rows are the restatement's staged rows
    want_rows, want_steps = N.rows(ring, cut, R.RING, position, stride, n_step, GAMMA, idx)
    href = torch.from_numpy(want_rows).to(DEV)
    ref = _critic(nets, NavReplay(href.data_ptr(), B), iota, eps, B)
    torch.cuda.synchronize()
    assert np.array_equal(steps.cpu().numpy(), want_steps) and want_steps.max() == n_step
    assert len(set(want_steps.tolist())) == n_step
    assert np.array_equal(bits(staged.cpu().numpy()), bits(want_rows))
    assert torch.equal(got["batch"], href) and torch.equal(got["lp"], ref["lp"])
    for key in ("dq", "es", "masks", "acts", "dz"):
        for k in range(2):
            assert torch.equal(got[key][k], ref[key][k]), (key, k)
    assert got["dq"][0].abs().max() > 0
    # the n-step formula in fp64: y = sum_j g^j r_j + g^m min Q'(s_{t+m}, a') (1 - done), through
    # mlp_ref's critic epoch on rows that carry R and 1 - g^(m-1) in fp64
    g = R.f32c(GAMMA)
    b64 = torch.from_numpy(want_rows).double()
    for b, (k0, m) in enumerate(zip(idx.tolist(), want_steps.tolist())):
        ks = [(k0 + j * stride) % R.RING for j in range(m)]
        b64[b, 4] = sum(g ** j * float(ring[k, 4]) for j, k in enumerate(ks))
        assert np.array_equal(want_rows[b, 5:7], ring[ks[-1], 5:7])
        b64[b, 7] = 1.0 if ring[ks[-1], 7] != 0 else 1.0 - g ** (m - 1)
    hp = nets["cr0"].hp
    mbits = [R.relu_bits(got["masks"][k], nh, hp, hidden, B) for k in range(2)]
    L = case["layers"]
    e = R.critic_epoch(L["ta"], [L["tc0"], L["tc1"]], [L["cr0"], L["cr1"]], b64, case["eps"],
                       mbits)
    one = R.critic_epoch(L["ta"], [L["tc0"], L["tc1"]], [L["cr0"], L["cr1"]],
                         case["rows"][case["idx"]], case["eps"], mbits)
    assert float((e["y"] - one["y"]).abs().max()) > 1.0  # not the one-step target
    for k in range(2):
        # q - y = dq B / 2: the target's error (and q's) relative to max(|q|, |y|)
        scale = max(float(e["q"][k].abs().max()), float(e["y"].abs().max()))
        err = float((got["dq"][k].double().cpu() * B / 2 - (e["q"][k] - e["y"])).abs().max())
        print(f"hidden {hidden} critic {k}: max |(q - y) - fp64| / scale {err / scale:.2e}")
        assert err / scale <= 2e-6


# ---------------------------------------------------------------- the trainer
def test_off_means_off(nav):
    from nav.trainer import VecTrainer
    snaps = []
    for kw in (dict(n_step=1), {}):
        tr = VecTrainer(device=DEV, **TRAINER, **kw)
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        assert tr.replay.cut is None and tr.td3.nstep_launches == 0 and not tr.td3.nstep_on()
        assert not hasattr(tr.td3, "staged") and not hasattr(tr.td3, "idx_iota")
        snaps.append(snapshot(tr, "moments", "env"))
        sd = tr.state_dict()
        assert "n_step" not in sd["meta"] and "cut" not in sd["replay"]
    assert _same(*snaps)
    assert snaps[0]["actor"].abs().max() > 0


def _filled(n_step=1, ticks=4, **kw):
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, **TRAINER, n_step=n_step, **kw)
    for _ in range(ticks):
        tr.collect()
    torch.cuda.synchronize()
    return tr


def test_horizon_one_is_plain(nav):
    """Every row cut: each staged row is its ring row, so two epochs through staged, the iota
    indices and the staged launch's counters end where the plain learner's do."""
    a, b = _filled(3), _filled(1)
    assert torch.equal(a.replay.rows, b.replay.rows) and _same(_params(a.td3), _params(b.td3))
    a.replay.cut.fill_(1)
    for tr in (a, b):
        tr.td3.td3_update(tr.replay, 2)
    torch.cuda.synchronize()
    assert a.td3.nstep_launches == 2 and b.td3.nstep_launches == 0
    assert (a.td3.steps == 1).all()
    assert _same(_params(a.td3), _params(b.td3)) and _same(_moments(a.td3), _moments(b.td3))
    # and with the marks cleared the horizons grow and the epoch is another one
    a.replay.cut.fill_(0)
    a.td3.td3_update(a.replay, 1)
    b.td3.td3_update(b.replay, 1)
    torch.cuda.synchronize()
    assert a.td3.steps.max() == 3 and not _same(_params(a.td3), _params(b.td3))


PER = dict(per_alpha=0.6, per_beta=0.4, per_eps=1e-6)


@pytest.mark.parametrize("per", [False, True], ids=["plain", "per"])
def test_epochs_follow_the_restatement(nav, per):
    """3 single epochs at n_step = 3 on a ring with seeded cut marks, beside a learner without
    n_step that is handed the restatement's staged rows by direct calls (train_critic's launches
    on a ring of the staged rows with idx = 0 .. B-1, then the actor launch on the real ring)."""
    from nav import config as K
    from nav._lib import stream_handle
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    tr = _filled(3, **(PER if per else {}))
    ring, t, B = tr.replay, tr.td3, 128
    rng = np.random.default_rng(5)
    rows = ring.rows.cpu().numpy()
    cut = ((rows[:, 7] != 0) | (rng.random(1024) < 0.2)).astype(np.uint8)
    ring.cut.copy_(torch.from_numpy(cut).to(DEV))
    ref = TD3(K.TD3Config(batch_size=B, num_epochs=1, net=K.NetConfig(hidden=64, n_hidden=2),
                          **(PER if per else {})), device=DEV, seed=tr.seed)
    assert _same(_params(t), _params(ref))
    ref._static()
    iota = torch.arange(B, dtype=torch.int64, device=DEV)
    host = lambda x: x.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    seen = set()
    for epoch in range(3):
        counter = t.update_counter
        pri = host(ring.pri) if per else None
        t.td3_update(ring, 1)
        torch.cuda.synchronize()
        idx = (P.sample(pri, 1024, B, tr.seed, counter, False) if per
               else N.draw(1024, B, tr.seed, counter))
        if per:
            assert np.array_equal(t.idx_c.cpu().numpy(), idx)
        staged, steps = N.rows(rows, cut, 1024, ring.position, 256, 3, GAMMA, idx)
        assert np.array_equal(t.steps.cpu().numpy(), steps), epoch
        assert np.array_equal(bits(t.staged.cpu().numpy()), bits(staged)), epoch
        seen |= set(steps.tolist())
        # the reference learner's epoch, as TD3._update issues it
        sring = ReplayRing(B, DEV, rows=torch.from_numpy(staged).to(DEV))
        sring.advance(B)
        s = stream_handle()
        assert ref.update_counter == counter
        g = ref._critic_rows(sring, iota, None, s, t.w_per if per else None)
        ref._step(g, s, None)
        # (a td3_update of one epoch is a policy epoch)
        ref.train_actor(ring, t.idx_a if per else None, soft_update=True)
        ref.update_counter += 1
        torch.cuda.synchronize()
        assert _same(_params(t), _params(ref)), epoch
        assert _same(_moments(t), _moments(ref)), epoch
        if per:
            assert torch.equal(t.td_abs1, ref.td_abs1) and torch.equal(t.td_abs2, ref.td_abs2)
            q = P.priority(t.td_abs1.cpu().numpy(), t.td_abs2.cpu().numpy(), PER["per_alpha"],
                           PER["per_eps"])
            dp = np.abs(host(ring.pri) - P.update(pri, idx, q)).max()
            print(f"epoch {epoch}: priority counts off by at most {dp}")
            assert dp <= 1  # the double pow's last bit, as test_gpu_per.py
    assert seen == {1, 2, 3}
    assert t.nstep_launches == 3 and ref.nstep_launches == 0
    assert t.per_launches == (9 if per else 0)


def test_checkpoint_resume_with_cut_marks(nav, tmp_path):
    from nav.trainer import VecTrainer
    a = VecTrainer(device=DEV, **TRAINER, n_step=3)
    for _ in range(5):
        a.step()
    # marks that only the checkpoint can carry over (these ticks are too few to end an episode)
    g = torch.Generator().manual_seed(2)
    a.replay.cut.copy_((torch.rand(1024, generator=g) < 0.3).to(torch.uint8).to(DEV))
    path = os.path.join(tmp_path, "nstep.pt")
    a.save(path)
    b = VecTrainer.load(path, device=DEV)
    assert b.td3.cfg.n_step == 3 and b.td3.nstep_on() and b.replay.stride == 256
    assert torch.equal(a.replay.cut, b.replay.cut) and 0 < int(b.replay.cut.sum()) < 1024
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert _same(_params(a.td3), _params(b.td3)) and _same(_moments(a.td3), _moments(b.td3))
    assert torch.equal(a.replay.rows, b.replay.rows) and torch.equal(a.replay.cut, b.replay.cut)
    assert torch.equal(a.td3.staged, b.td3.staged) and torch.equal(a.td3.steps, b.td3.steps)
    assert int(a.td3.steps.max()) > 1
    for k in a.ENV_STATE:
        assert torch.equal(getattr(a.env, k), getattr(b.env, k)), k
    # a checkpoint written with the feature off loads as n_step = 1
    plain = VecTrainer(device=DEV, demos=False, **TRAINER)
    plain.step()
    off = VecTrainer.from_state_dict(plain.state_dict(), device=DEV)
    assert off.td3.cfg.n_step == 1 and not off.td3.nstep_on() and off.replay.cut is None


class _Hook:
    world_size = 1

    def __call__(self, bucket):
        return None


@pytest.mark.parametrize("kw", [dict(demo_fraction=0.25), dict(bc_weight=1.0),
                                dict(demo_fraction=0.25, bc_weight=1.0),
                                dict(grad_hook=_Hook()), dict(overlap_collect=True)],
                         ids=["demo_fraction", "bc_weight", "both", "grad_hook", "overlap_collect"])
def test_rejected_combinations(nav, kw):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="multi-step returns"):
        VecTrainer(device=DEV, demos=False, **TRAINER, n_step=3, **kw)


def test_rejected_population_member_and_bad_n_step(nav):
    from nav.population import PopulationTrainer
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="multi-step returns"):
        PopulationTrainer([{}, {"n_step": 3}], envs_per_member=64, hidden=64, batch=64,
                          envs_per_group=64, demos=False, device=DEV)
    for bad in (0, N.NSTEP_MAX + 1):
        with pytest.raises(ValueError, match="n_step"):
            VecTrainer(device=DEV, demos=False, n_step=bad, **TRAINER)
    # prioritised replay is allowed
    tr = VecTrainer(device=DEV, demos=False, n_step=2, **PER, **TRAINER)
    assert tr.replay.cut is not None and tr.replay.pri is not None


def test_ring_without_marks_or_stride_refuses_an_n_step_learner(nav):
    from nav import config as K
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    t = TD3(K.TD3Config(batch_size=64, net=K.NetConfig(hidden=64, n_hidden=2), n_step=3),
            device=DEV)
    ring = ReplayRing(256, DEV)
    ring.advance(256)
    with pytest.raises(ValueError, match="cut marks"):
        t.td3_update(ring, 1)
    ring = ReplayRing(256, DEV, cuts=True)
    ring.advance(256)
    with pytest.raises(ValueError, match="stride"):
        t.td3_update(ring, 1)
    assert t.nstep_launches == 0
