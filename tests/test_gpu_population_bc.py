"""Populations that learn from demonstrations, on the GPU: nav_td3_mix_idx_pop and
nav_td3_actor_rows_bc_pop against the single-member entry points on the same arguments (which
tests/test_gpu_bc.py pins to the host Philox and to fp64), the batched learner's epochs against
lone TD3 objects, and PopulationTrainer with per-member demo_fraction / bc_weight / q_weight
against VecTrainer, against learner="members", in mixed populations, with the keys off, through
an exploit and through pretrain_bc. Every comparison but the fp64 one is bitwise."""
import pytest
import torch

import bc_ref as BR
import mlp_ref as R
import pop_bc_ref as PB
import pop_support as PS
from gpu_support import nav  # noqa: F401
from launches import device_net as _device_net
from pop_support import equal_tree, learner_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP, FILL, N_TAIL, COUNTER = PB.CAP, PB.FILL, PB.N_TAIL, PB.COUNTER


def _nan_fill(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(0x5A5A if t.dtype == torch.int16 else -1)


def tailed_ring(m, storage=None):
    """pop_support.make_ring with a tail of N_TAIL demonstration rows behind the ring."""
    return PS.make_ring(m, tail=N_TAIL, storage=storage, cap=CAP, fill=FILL)


class KernelCase:
    """P members' learners (own seeds, so own weights) on tailed rings, their nav_td3_member
    array with every member's index arrays set, a nav_td3_member_bc array of the given B_demo and
    weights and the BC table built from both."""

    OUT = ("batch2", "q1", "da", "bc_part", "acts_a", "dz_a", "mask_a", "mask1", "eslab_a")

    def __init__(self, hidden, nh, B, b_demos, weights=None, fp64_member=None):
        from nav import config as K
        from nav._lib import NavTd3MemberBc, lib, ptr
        from nav.population import PopulationLearner
        from nav.td3 import TD3
        P = self.P = len(b_demos)
        self.B, self.b_demos = B, list(b_demos)
        self.weights = list(weights or [(1.0, 0.5 if b else 0.0) for b in b_demos])
        self.td3, self.rings = [], []
        for m in range(P):
            cfg = K.TD3Config(batch_size=B, net=K.NetConfig(hidden=hidden, n_hidden=nh))
            nets, storage = {}, None
            if m == fp64_member:
                self.case, storage = PB.fp64_member_rows()
                nets = dict(actor=_device_net(self.case["layers"]["actor"], 2, 2, hidden, nh),
                            critic1=_device_net(self.case["layers"]["cr0"], 4, 1, hidden, nh))
            t = TD3(cfg, device=DEV, seed=PB.member_seed(m), **nets)
            t._static()
            t.update_counter = COUNTER
            self.td3.append(t)
            self.rings.append(tailed_ring(m, storage))
        self.learner = PopulationLearner(self.td3, self.rings)
        assert self.learner.bc_table is None  # no member's cfg has the feature on
        self.learner.inject(idx_critic=[t.idx_c for t in self.td3],
                            idx_actor=[t.idx_a for t in self.td3])
        self.members = self.learner.members
        self.bc = (NavTd3MemberBc * P)(*[
            NavTd3MemberBc(b, N_TAIL, q, w, t.idx_c.data_ptr(), t.idx_a.data_ptr(),
                           t.bc_part.data_ptr())
            for t, b, (q, w) in zip(self.td3, self.b_demos, self.weights)])
        L = lib()
        self.table = torch.zeros(L.nav_td3_pop_bc_table_bytes(P), dtype=torch.uint8, device=DEV)
        L.nav_td3_pop_bc_table_build(self.members, self.bc, P, B, ptr(self.table), None)

    def prefill(self):
        for t in self.td3:
            for k in self.OUT + ("idx_c", "idx_a"):
                _nan_fill(getattr(t, k))

    def outputs(self, m):
        torch.cuda.synchronize()
        return {k: getattr(self.td3[m], k).clone() for k in self.OUT + ("idx_c", "idx_a")}

    def run_pop(self, plain=False):
        """The mix launch and the BC actor launch (plain: nav_td3_actor_rows_pop) for all
        members; every member's outputs."""
        from nav._lib import lib, ptr
        L = lib()
        self.prefill()
        L.nav_td3_mix_idx_pop(self.members, self.bc, self.P, self.B, ptr(self.table), FILL,
                              COUNTER, 1, None)
        if plain:
            L.nav_td3_actor_rows_pop(self.members, self.P, self.B, ptr(self.learner.table), FILL,
                                     COUNTER, None)
        else:
            L.nav_td3_actor_rows_bc_pop(self.members, self.bc, self.P, self.B, ptr(self.table),
                                        FILL, COUNTER, None)
        return [self.outputs(m) for m in range(self.P)]

    def run_lone(self, m):
        """Member m's own nav_td3_mix_idx and nav_td3_actor_rows_bc with the same size and
        counter, into the same (prefilled) buffers."""
        from nav._lib import lib, ptr
        t, seed = self.td3[m], PB.member_seed(m)
        self.prefill()
        lib().nav_td3_mix_idx(FILL, self.B, self.b_demos[m], CAP, N_TAIL, seed & 0xFFFFFFFF,
                              seed >> 32, COUNTER, ptr(t.idx_c), ptr(t.idx_a), None)
        q, w = self.weights[m]
        t._actor_rows_bc(True, t._replay_ref(self.rings[m]), FILL, t.idx_a, self.b_demos[m], q,
                         w, None)
        return self.outputs(m)


def same_nan(a, b):
    """Bitwise equality of two output dicts, NaN prefill included."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            bad.append(k)
    return bad


# ---- nav_td3_mix_idx_pop ----
MIX_B, MIX_DEMO = 100, (0, 7, 100)


@pytest.fixture(scope="module")
def first_case(nav):
    """hidden 64 x 2, B = 100, P = 3: four 32-row blocks, the last of 4 rows; member 2's every
    row a demonstration row; member 1 carries tests/bc_ref.py's weights and rows."""
    return KernelCase(64, 2, MIX_B, MIX_DEMO, [(1.0, 0.0), (1.0, 0.5), (0.25, 3.0)],
                      fp64_member=PB.FP64["member"])


def test_mix_idx_pop_is_each_members_mix_idx(nav, first_case, orc):
    from nav._lib import lib, ptr
    kc = first_case
    got = kc.run_pop()
    for m in range(kc.P):
        want = kc.run_lone(m)
        assert torch.equal(got[m]["idx_c"], want["idx_c"]), m
        assert torch.equal(got[m]["idx_a"], want["idx_a"]), m
        b = MIX_DEMO[m]
        tail = got[m]["idx_c"][:b]
        assert b == 0 or (int(tail.min()) >= CAP and int(tail.max()) < CAP + N_TAIL)
        assert b == MIX_B or int(got[m]["idx_c"][b:].max()) < FILL
    # the members draw from their own seeds
    assert not torch.equal(got[0]["idx_c"][7:], got[1]["idx_c"][7:])
    # member 1's demonstration rows against the host Philox, the formula of
    # tests/test_gpu_bc.py::test_mix_idx_demonstration_rows_vs_host_philox
    seed = PB.member_seed(1)
    for y, k in enumerate(("idx_c", "idx_a")):
        want = PB.host_mix_idx(orc, seed, MIX_B, 7, FILL, CAP, N_TAIL, COUNTER, actor=bool(y))
        assert got[1][k].tolist() == want
    # actor_too = 0 leaves idx_actor alone
    kc.prefill()
    lib().nav_td3_mix_idx_pop(kc.members, kc.bc, kc.P, kc.B, ptr(kc.table), FILL, COUNTER, 0, None)
    for m in range(kc.P):
        o = kc.outputs(m)
        assert torch.equal(o["idx_c"], got[m]["idx_c"]) and bool((o["idx_a"] == -1).all())


# ---- nav_td3_actor_rows_bc_pop ----
def check_pop_is_lone(kc):
    got = kc.run_pop()
    for m in range(kc.P):
        want = kc.run_lone(m)
        bad = same_nan(got[m], want)
        assert not bad, (m, bad)
        assert bool(torch.isfinite(got[m]["da"]).all() and torch.isfinite(got[m]["q1"]).all())
        assert torch.equal(got[m]["batch2"], kc.rings[m].storage[got[m]["idx_a"]])
        tm = 32 if kc.B <= 16384 else 64
        first_free = (kc.b_demos[m] + tm - 1) // tm
        part = got[m]["bc_part"]
        assert bool((part[first_free:] == 0).all()) and bool((part[:first_free] > 0).all())
    for m in range(1, kc.P):  # a condition: another member's entry cannot pass
        assert not torch.equal(got[0]["da"], got[m]["da"])
    return got


def test_actor_rows_bc_pop_first_case(nav, first_case):
    got = check_pop_is_lone(first_case)
    # the B_demo = 0, bc_weight = 0, q_weight = 1 member is also nav_td3_actor_rows_pop's
    plain = first_case.run_pop(plain=True)
    bad = [k for k in same_nan(got[0], plain[0]) if k != "bc_part"]
    assert not bad, bad
    assert bool((got[0]["bc_part"] == 0).all()) and bool(plain[0]["bc_part"].isnan().all())
    # a condition: the plain launch is not the BC form for a member with demonstration rows
    assert "da" in same_nan(got[1], plain[1])


ROWS_CASES = [
    (64, 2, 100, (40, 33)),      # the demonstration boundary inside the second block, and one past
    (32, 1, 100, (7, 64)),       # one hidden layer, CBM = 0
    (200, 3, 100, (25, 0)),      # hp 224, the middle layers saved
    (64, 2, 16421, (4105, 0)),   # above kSmallRows: 64-row blocks, a ragged last block
    (256, 2, 2112, (528,) * 8),  # more workgroups than CUs, members co-resident
]


@pytest.mark.parametrize("hidden,nh,B,b_demos", ROWS_CASES,
                         ids=[f"h{h}x{n}_b{b}_p{len(d)}" for h, n, b, d in ROWS_CASES])
def test_actor_rows_bc_pop_is_each_members_actor_rows_bc(nav, hidden, nh, B, b_demos):
    """Every output of member m (batch_actor, q, da, bc_part, the saved acts / dz, both mask
    buffers, the edge slabs; the rows a launch leaves alone stay NaN in both) equals
    nav_td3_actor_rows_bc on that member's arguments with the same size and counter."""
    check_pop_is_lone(KernelCase(hidden, nh, B, b_demos))


def test_actor_rows_bc_pop_vs_fp64(nav, first_case):
    """The B_demo = 7 member's da and bc_part (and q) against tests/bc_ref.py's actor_epoch_bc in
    fp64 with the kernel's ReLU bits injected, at the bars tests/test_gpu_bc.py applies to the
    single-member form (mlp_ref.bar: row quantities 2e-6 of scale, the BC sum as a cross-row sum
    1e-5, each at least 8 x the fp32 chain's own error); the band cap is established on the CPU
    in tests/test_population_bc_cpu.py."""
    kc, f = first_case, PB.FP64
    m, hidden, nh, B, b_demo = f["member"], f["hidden"], f["nh"], f["B"], f["b_demo"]
    o = kc.run_pop()[m]
    q_w, bc_w = kc.weights[m]
    hp = kc.td3[m].actor_network.hp
    rows_a = kc.rings[m].storage[o["idx_a"]].cpu()
    assert torch.equal(o["batch2"].cpu(), rows_a)
    la, lc = kc.case["layers"]["actor"], kc.case["layers"]["cr0"]
    bits_a = R.relu_bits(o["mask_a"], nh, hp, hidden, B)
    bits_c = R.relu_bits(o["mask1"], nh, hp, hidden, B)
    args = (la, lc, rows_a, bits_a, bits_c, b_demo, q_w, bc_w)
    ref, f32 = BR.actor_epoch_bc(*args), BR.actor_epoch_bc(*args, dtype=torch.float32)
    inside, entries = R.relu_band(la, rows_a[:, :2], ref["zs_a"], bits_a)
    bar_a = R.bar("a", R.rel_err(f32["a"], ref["a"])) * float(ref["a"].abs().max())
    extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ lc[0][0][:, 2:4].double().abs().t()
    i2, e2 = R.relu_band(lc, ref["x_c"], ref["zs_c"], bits_c, extra0=extra)
    R.assert_band_cap(inside + i2, entries + e2)
    da = o["da"].cpu()
    dev = dict(da=da, loss_bc=o["bc_part"].cpu().double().sum().reshape(1), da_demo=da[:b_demo],
               da_rest=da[b_demo:], q=o["q1"].cpu())
    keep = lambda d: {k: v for k, v in BR.bc_quantities(d).items() if k in dev}  # noqa: E731
    over = R.ParityLog().judge(hp, nh, "actor_rows_bc_pop", R.compare(dev, keep(ref), keep(f32)))
    assert not over, over


# ---- the batched learner's epochs ----
LEARN = [(0.25, 1.0, 1.0), (0.5, 0.5, 0.25), (1.0, 3.0, 0.5)]  # demo_fraction, bc_weight, q_weight


def bc_td3(m, B, epochs, splits=None):
    """pop_support.make_td3 at hidden 64 x 2 with member m's demonstration weights, pop_bc_ref's
    seed, and the default smoothing noise and action bound for every member."""
    from nav import config as K
    f, w, q = LEARN[m]
    d = K.TD3Config()
    return PS.make_td3(m, 64, 2, B, epochs, splits, seed=PB.member_seed(m), demo_fraction=f,
                       bc_weight=w, q_weight=q, policy_noise=d.policy_noise,
                       noise_clip=d.noise_clip, max_action=d.max_action)


def bc_state(t):
    s = learner_state(t)
    s.update(bc_part=t.bc_part.clone(), idx_c=t.idx_c.clone(), idx_a=t.idx_a.clone(),
             actor_loss=t.actor_loss_value(), bc_loss=t.bc_loss_value(),
             critic_loss=tuple(t.critic_loss_values()))
    return s


def test_epochs_distinct_members(nav):
    """P = 3 members with their own seeds, learning rates and three weights, B = 128, three
    epochs (policy, critic only, policy): per member the six nets, packed images, moments, both
    sampled batches, bc_part and the loss values equal a lone TD3 through _update_bc with the
    batched run's split counts; one mix launch per epoch for the whole population."""
    from nav.population import PopulationLearner
    B, P = 128, 3
    rings = [tailed_ring(m) for m in range(P)]
    td3 = [bc_td3(m, B, 3) for m in range(P)]
    learner = PopulationLearner(td3, rings)
    assert learner.bc_table is not None
    learner.update(3)
    torch.cuda.synchronize()
    got = [bc_state(t) for t in td3]
    assert learner.mix_launches == 3 and all(t.mix_launches == 0 for t in td3)
    for m in range(P):
        t = bc_td3(m, B, 3, splits=learner.wgrad_splits)
        t.td3_update(rings[m], 3)
        torch.cuda.synchronize()
        assert t.mix_launches == 3 and t.b_demo() == round(LEARN[m][0] * B)
        equal_tree(got[m], bc_state(t), f"member {m}")
        assert got[m]["bc_loss"] > 0 and got[m]["adam"]["actor"]["t"] == 2
        assert torch.equal(got[m]["batch2"], rings[m].storage[got[m]["idx_a"]])
        assert int(got[m]["idx_a"][:t.b_demo()].min()) >= CAP
    for m in range(1, P):
        assert not torch.equal(got[0]["params"]["actor"], got[m]["params"]["actor"])


# ---- the trainer ----
TRAINER = dict(hidden=64, n_hidden=2, batch=128, updates_per_step=2, seed=1234,
               envs_per_group=128)
ON = {"demo_fraction": 0.25, "bc_weight": 1.0}


def tailed_state(tr, m):
    """Member m's env slice, its ring with the tail and its learner."""
    return PS.member_state(tr, m, tail=True)


def run_trainer(members, steps=3, **kw):
    from nav.population import PopulationTrainer
    tr = PopulationTrainer(members, envs_per_member=256, device=DEV, **TRAINER, **kw)
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return tr, [tailed_state(tr, m) for m in range(len(members))]


@pytest.fixture(scope="module")
def vec_run(nav):
    from nav.trainer import VecTrainer
    vt = VecTrainer(n_envs=256, device=DEV, **TRAINER, **ON)
    for _ in range(3):
        vt.step()
    torch.cuda.synchronize()
    sd = vt.state_dict()
    return vt, {"env": sd["env"],
                "replay": {"rows": vt.replay.storage.cpu(), "position": vt.replay.position,
                           "size": vt.replay.size},
                "td3": sd["td3"], "steps": sd["meta"]["steps"]}


@pytest.mark.parametrize("learner", ["members", "batched"])
def test_trainer_one_member_is_vectrainer(nav, vec_run, learner):
    """One member with demo_fraction 0.25 and bc_weight 1 after 3 steps equals VecTrainer with the
    same arguments: env state, ring including the tail, every parameter and moment."""
    vt, want = vec_run
    pt, st = run_trainer([dict(ON)], learner=learner)
    assert pt.ring_rows.shape == (1, vt.replay.capacity + vt.replay.tail.shape[0], 8)
    assert vt.replay.tail.shape[0] > 0 and vt.td3.mix_launches == 6
    equal_tree(st[0], want)
    launches = pt.learner.mix_launches if learner == "batched" else pt.td3[0].mix_launches
    assert launches == 6 and pt.td3[0].update_counter == 6
    assert pt.td3[0].bc_loss_value() == vt.td3.bc_loss_value() > 0
    assert pt.td3[0].actor_loss_value() == vt.td3.actor_loss_value()


PAIR = [{"demo_fraction": 0.25, "bc_weight": 1.0, "q_weight": 0.5},
        {"demo_fraction": 0.5, "bc_weight": 0.5}]


@pytest.fixture(scope="module")
def pair_run(nav):
    return run_trainer(PAIR, learner="batched")


def test_trainer_batched_is_members_and_isolates(nav, pair_run):
    """P = 2 with different weights: batched equals members (with the batched run's split counts)
    after 3 steps; each member's tail holds its own groups' demonstrations; changing only member
    1's bc_weight leaves member 0 bit-identical and changes member 1's actor."""
    bt, b = pair_run
    mt, a = run_trainer(PAIR, learner="members", wgrad_splits=bt.learner.wgrad_splits)
    equal_tree(b, a)
    assert bt.learner.mix_launches == 6 and [t.mix_launches for t in mt.td3] == [6, 6]
    st, ac, gl = bt._cem
    from nav.demo_replay import DemoReplay
    for m in range(2):
        sl = slice(6 * m, 6 * m + 6)  # 2 groups of 128 envs x 3 demonstrations
        want = DemoReplay(st[sl], ac[sl], gl[sl], bt.params[m]).rows0
        assert torch.equal(bt.rings[m].tail, want) and want.shape[0] == bt.rings[m].tail.shape[0]
    assert not torch.equal(bt.rings[0].tail, bt.rings[1].tail)
    _, c = run_trainer([PAIR[0], {**PAIR[1], "bc_weight": 2.0}], learner="batched")
    equal_tree(c[0], b[0])
    assert not torch.equal(c[1]["td3"]["actor"]["params"], b[1]["td3"]["actor"]["params"])


def test_trainer_mixed_population(nav):
    """P = 2, member 0 without the keys: it ends bit-identical to member 0 of a population where
    nobody has them (same split counts), in one launch per kernel with member 1's BC term."""
    mt, mixed = run_trainer([{}, dict(ON)], learner="batched")
    pt, plain = run_trainer([{}, {}], learner="batched")
    assert mt.learner.wgrad_splits == pt.learner.wgrad_splits
    assert mt.learner.mix_launches == 6 and pt.learner.mix_launches == 0
    cap = pt.ring_rows.shape[1]
    got = dict(mixed[0])
    got["replay"] = dict(got["replay"], rows=got["replay"]["rows"][:cap])
    equal_tree(got, plain[0])
    assert not torch.equal(mixed[1]["td3"]["actor"]["params"], plain[1]["td3"]["actor"]["params"])
    assert mt.td3[0].actor_loss_value() == pt.td3[0].actor_loss_value()


@pytest.mark.parametrize("learner", ["members", "batched"])
def test_trainer_keys_off(nav, learner):
    tr, _ = run_trainer([{}, {"critic_lr": 1e-4}], learner=learner)
    cap = tr.rings[0].capacity
    assert tr.ring_rows.shape == (2, cap, 8) and all(r.tail.shape[0] == 0 for r in tr.rings)
    assert not tr.bc and tr.demo_replays is None
    assert all(t.mix_launches == 0 for t in tr.td3)
    if learner == "batched":
        assert tr.learner.bc_table is None and tr.learner.bc_members is None
        assert tr.learner.mix_launches == 0


def test_exploit_hands_over_the_values_and_keeps_the_tail(nav, pair_run):
    """exploit([0], [1]): member 1 takes member 0's three values and keeps its own tail; batched
    still equals members over 2 further steps."""
    splits = pair_run[0].learner.wgrad_splits
    ends = []
    for kw in (dict(learner="batched"), dict(learner="members", wgrad_splits=splits)):
        tr, _ = run_trainer(PAIR, **kw)
        tail = tr.rings[1].tail.clone()
        tr.exploit([0], [1])
        for k in ("demo_fraction", "bc_weight", "q_weight"):
            assert tr.member_value(1, k) == tr.member_value(0, k) == PAIR[0].get(k, 1.0)
        assert torch.equal(tr.rings[1].tail, tail)
        assert torch.equal(tr.td3[1].actor_network.params, tr.td3[0].actor_network.params)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        assert torch.equal(tr.rings[1].tail, tail)
        ends.append([tailed_state(tr, m) for m in range(2)])
    equal_tree(ends[0], ends[1])
    with pytest.raises(KeyError, match="cannot be explored"):
        tr.exploit([0], [1], explore={"demo_fraction": (0.0, 1.0)})


def test_explore_cannot_leave_a_weight_on_no_rows(nav):
    """A clone of a member without demonstration rows cannot be handed a bc_weight above 0."""
    tr, _ = run_trainer([{}, dict(ON)], steps=1, learner="batched")
    with pytest.raises(ValueError, match="bc_weight needs demonstration rows"):
        tr.exploit([0], [1], explore={"bc_weight": (0.5, 4.0)})
    ev = tr.exploit([1], [0], explore={"bc_weight": (0.0, 4.0)})
    assert ev[0]["explored"]["bc_weight"] in (0.8, 1.25) and tr.td3[0].b_demo() == 32


def test_population_pretrain_bc_lowers_every_members_loss(nav):
    from nav.population import PopulationTrainer
    tr = PopulationTrainer([dict(ON), {}], envs_per_member=256, device=DEV, learner="batched",
                           **TRAINER)
    before = tr.bc_loss()
    assert before == tr.bc_loss() and len(before) == 2
    tr.pretrain_bc(20, lr=1e-3)
    after = tr.bc_loss()
    print(f"bc_loss {before} -> {after}")
    assert all(a < b for a, b in zip(after, before))
    for t in tr.td3:
        assert torch.equal(t.target_actor.params, t.actor_network.params)
        assert t.actor_optimizer.lr == t.cfg.actor_lr and t.mix_launches == 20
    tr.step()  # training goes on from the cloned actors
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.actor_network.params).all()) for t in tr.td3)
