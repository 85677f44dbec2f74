"""Learning from demonstrations on the GPU: nav_demo_transitions against its numpy restatement,
nav_td3_mix_idx against the host Philox, the behaviour-cloning forms of the actor row kernel
(nav_td3_actor_rows_bc) against the fp64 chain of tests/bc_ref.py and bit for bit against the
plain form, and the trainer's demonstration mix, checkpoint and BC pretraining.

Bars: tests/mlp_ref.py's (row quantities 2e-6 of scale, cross-row sums 1e-5, each at least 8 x
the fp32 chain's own error); the BC loss counts as a sum. The conditions the comparisons rely on
(the ReLU band cap for the BC cases, 200 pure-BC Adam steps lowering the loss) are established on
the CPU in tests/test_bc_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc_ref as BR
import launches as LN
import mlp_ref as R
from gpu_support import equal_nan as _equal_nan, ids as _ids, nav  # noqa: F401
from launches import nan as _nan
from pop_support import same as _same, snapshot
from trace_support import assert_demo_rows, demo_cases

pytestmark = pytest.mark.gpu
DEV = R.DEV
SEED = LN.SEED
NAN = float("nan")
BIG = 16421  # 64-row blocks, the last one partial


# ---- nav_demo_transitions ----
def _demonstrations(n, T, seed):
    """n paths of T states that walk from a random start to within ~1 of their goal, the first
    one ending well inside the goal threshold and the last one far outside; raw actions up to
    +-10 (beyond the +-5 clamp of frame 1)."""
    g = np.random.RandomState(seed)
    goal = 5 + 90 * g.random_sample((n, 2))
    start = 100 * g.random_sample((n, 1, 2))
    t = np.linspace(1.0, 0.0, T).reshape(1, T, 1)
    st = goal[:, None] + (start - goal[:, None]) * t + g.standard_normal((n, T, 2)) * 0.3
    st[-1] += 40.0
    ac = g.uniform(-10, 10, (n, T, 2))
    return st.astype(np.float32), ac.astype(np.float32), goal


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("n,T", [(2, 5), (6, 200)])
def test_demo_transitions_bit_equal_to_the_restatement(nav, n, T, frame):
    from nav._lib import lib, params_struct, ptr, stream_handle
    from nav.demo_replay import transitions_ref
    st, ac, goal = _demonstrations(n, T, 10 * n + T)
    want = transitions_ref(st, ac, goal, frame)
    assert (want[:, 4] == 50.0).any() and (want[:, 4] < -5.0).any()  # both reward branches
    rows = _nan(n * (T - 1), 8)
    assert lib().nav_demo_transitions(
        C.byref(params_struct()), n, T, ptr(torch.tensor(st, device=DEV)),
        ptr(torch.tensor(ac, device=DEV)), ptr(torch.tensor(goal, device=DEV)), frame, ptr(rows),
        stream_handle()) == 0
    got = rows.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[:, 7].sum() == n and (got[T - 2::T - 1, 7] == 1).all()
    if frame == 1:
        # residual + baseline = clamp(a), up to the two f32 roundings
        assert np.abs(got[:, 2:4].astype(np.float64) + got[:, 0:2]).max() <= 5.0 + 1e-4


@pytest.mark.parametrize("case", range(4), ids=["trace", "trace_branches", "trace_branches_field",
                                                 "hand"])
def test_demo_transitions_vs_reference_pushes(nav, case):
    """nav_demo_transitions (frame 0) on the demonstrations the reference drew against the rows
    its process_demonstration pushed (the demo ticks of the three trace fixtures, 3 x 199 each,
    and a hand-made path that ends inside the goal radius): state, action, next-state and done
    columns equal, the reward equal or one float32 ulp from float32(push_r), rows inside
    the goal radius exactly 50."""
    from nav._lib import lib, params_struct, ptr, stream_handle
    name, st, ac, goals, want, rew = demo_cases()[case]
    n, T = st.shape[:2]
    rows = _nan(n * (T - 1), 8)
    assert lib().nav_demo_transitions(
        C.byref(params_struct()), n, T, ptr(torch.tensor(st, device=DEV)),
        ptr(torch.tensor(ac, device=DEV)), ptr(torch.tensor(goals, device=DEV)), 0, ptr(rows),
        stream_handle()) == 0
    n_goal, n_ulp = assert_demo_rows(rows.cpu().numpy(), want, rew)
    print(f"{name}: {n_goal} goal rows, {n_ulp} rewards one ulp off")
    # a condition on the inputs: the goal-reward branch is taken (the field trace's CEM
    # demonstrations never enter the radius; the hand-made path is there for that)
    assert n_goal >= 2 or name == "trace_branches_field.npz"


# ---- nav_td3_mix_idx ----
MIX = dict(B=100, size=500, n_demo=37, demo_base=500, counter=3)


def _mix(b_demo, both=True):
    from nav._lib import lib, ptr, stream_handle
    ic = torch.full((MIX["B"],), -1, dtype=torch.int64, device=DEV)
    ia = torch.full((MIX["B"],), -1, dtype=torch.int64, device=DEV)
    assert lib().nav_td3_mix_idx(MIX["size"], MIX["B"], b_demo, MIX["demo_base"], MIX["n_demo"],
                                 SEED & 0xFFFFFFFF, SEED >> 32, MIX["counter"], ptr(ic),
                                 ptr(ia) if both else None, stream_handle()) == 0
    torch.cuda.synchronize()
    return ic, ia


def _rows_batches(nets, dev, idx_c, idx_a):
    """The `batch` outputs of the existing nav_td3_critic_rows / nav_td3_actor_rows launches at
    MIX's counter with the given indices (None: the kernels' own Philox draw), nothing saved."""
    dev = dict(dev, idx=idx_c, idx_a=idx_a, size=MIX["size"])
    kw = dict(fill=NAN, save=False, counter=MIX["counter"])
    bc = LN.critic_rows(nets, dev, MIX["B"], **kw)["batch"]
    ba = LN.actor_rows(nets, dev, MIX["B"], form="plain", **kw)["batch"]
    torch.cuda.synchronize()
    return bc, ba


def test_mix_idx_without_demonstrations_is_the_kernels_own_draw(nav):
    """B_demo = 0: idx_critic / idx_actor fed to the existing row kernels give the batch the
    same launches draw themselves with idx = NULL at the same counter, bit for bit."""
    nets, dev = LN.device_epoch(R.epoch_case(64, 2, MIX["B"]))
    dev["rows"][:, 0] = torch.arange(R.RING, device=DEV)  # every row distinct
    ic, ia = _mix(0)
    assert int(ic.min()) >= 0 and int(ic.max()) < MIX["size"] and not torch.equal(ic, ia)
    got = _rows_batches(nets, dev, ic, ia)
    want = _rows_batches(nets, dev, None, None)
    for g, w, idx in zip(got, want, (ic, ia)):
        assert torch.equal(g, w)
        assert torch.equal(g[:, 0].long(), idx)
    only_c, untouched = _mix(0, both=False)  # a NULL output is left alone
    assert torch.equal(only_c, ic) and bool((untouched == -1).all())


@pytest.mark.parametrize("b_demo", [7, 100])
def test_mix_idx_demonstration_rows_vs_host_philox(nav, orc, b_demo):
    """Rows < B_demo: demo_base + ((w.x * n_demo) >> 32) of the oracle's Philox at ctr = (b, 0,
    NAV_TAG_DEMO = 7, 2 * counter [+ 1]), inside the tail; the remaining rows as with B_demo = 0."""
    ic, ia = _mix(b_demo)
    ic0, ia0 = _mix(0)
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for y, (got, plain) in enumerate(((ic, ic0), (ia, ia0))):
        want = [MIX["demo_base"] + ((orc.philox((b, 0, 7, 2 * MIX["counter"] + y), key)[0] *
                                     MIX["n_demo"]) >> 32) for b in range(b_demo)]
        assert got[:b_demo].tolist() == want
        assert 500 <= min(want) and max(want) < 537
        assert torch.equal(got[b_demo:], plain[b_demo:])
    assert not torch.equal(ic[:b_demo], ia[:b_demo])


# ---- the BC forms of the actor row kernel ----
def _bc_setup(hidden, nh, B, b_demo):
    case = BR.bc_case(hidden, nh, B, b_demo)
    return (case, *LN.device_epoch(case))


def _actor_rows_bc(nets, dev, B, b_demo, q_weight, bc_weight, critic=True, plain=False):
    """nav_td3_actor_rows_bc (plain: nav_td3_actor_rows) into NaN-prefilled buffers; then the
    weight gradients and the reduce into the actor's flat gradient `g`."""
    if plain:
        o = LN.actor_rows(nets, dev, B, form="plain", fill=NAN)
    else:
        o = LN.actor_rows(nets, dev, B, form="bc", fill=NAN, b_demo=b_demo, q_weight=q_weight,
                         bc_weight=bc_weight, critic=critic)
    o["g"], = LN.flat_grads([nets["actor"]], o, fill=NAN)
    torch.cuda.synchronize()
    return o


def _judge_bc(case, nets, o, hidden, nh, B, b_demo, q_weight, bc_weight, critic):
    """The launch's outputs against actor_epoch_bc in fp64 with the kernel's ReLU bits injected;
    returns the quantities over their bar (every figure is printed)."""
    hp = nets["actor"].hp
    rows_a = case["rows"][case["idx_a"]]
    assert torch.equal(o["batch"].cpu(), rows_a)
    la, lc = case["layers"]["actor"], case["layers"]["cr0"] if critic else None
    bits_a = R.relu_bits(o["ma"], nh, hp, hidden, B)
    bits_c = R.relu_bits(o["mc"], nh, hp, hidden, B) if critic else None
    args = (la, lc, rows_a, bits_a, bits_c, b_demo, q_weight, bc_weight)
    ref, f32 = BR.actor_epoch_bc(*args), BR.actor_epoch_bc(*args, dtype=torch.float32)
    inside, entries = R.relu_band(la, rows_a[:, :2], ref["zs_a"], bits_a)
    if critic:
        bar_a = R.bar("a", R.rel_err(f32["a"], ref["a"])) * float(ref["a"].abs().max())
        extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ \
            lc[0][0][:, 2:4].double().abs().t()
        i2, e2 = R.relu_band(lc, ref["x_c"], ref["zs_c"], bits_c, extra0=extra)
        inside, entries = inside + i2, entries + e2
    R.assert_band_cap(inside, entries)
    part = o["part"].cpu()
    assert bool(torch.isfinite(part).all())
    # a block without demonstration rows reports exactly 0
    tm = 32 if B <= 16384 else 64  # the row blocks' height (nav_mlp_row_blocks)
    assert o["nblk"] == (B + tm - 1) // tm
    first_free = (b_demo + tm - 1) // tm
    assert bool((part[first_free:] == 0).all()) and bool((part[:first_free] > 0).all())
    d = dict(da=o["da"].cpu(), loss_bc=part.double().sum().reshape(1))
    if 0 < b_demo < B:
        d.update(da_demo=d["da"][:b_demo], da_rest=d["da"][b_demo:])
    if critic:
        d["q"] = o["q"].cpu()
    d.update(R.flat_grad_tensors(o["g"].cpu(), 2, 2, hidden, hp, nh))
    log = R.ParityLog()
    return log.judge(hp, nh, "actor_rows_bc" if critic else "actor_rows_bc_only",
                     R.compare(d, BR.bc_quantities(ref), BR.bc_quantities(f32)))


BC_SHAPES = [(24, 1), (90, 2), (200, 3), (256, 2)]
BC_CASES = [(h, nh, B, bd) for h, nh in BC_SHAPES for B in (33, 100) for bd in (0, 7, B)]
BC_CASES.append((150, 2, BIG, 4100))  # 64-row blocks: one mixes both kinds of row, the last partial


@pytest.mark.parametrize("hidden,nh,B,b_demo", BC_CASES, ids=_ids(BC_CASES))
def test_actor_rows_bc_vs_fp64(nav, hidden, nh, B, b_demo):
    """TD3_BC form, q_weight = 1, bc_weight = 0.5 (0 where no row is a demonstration row): batch
    == rows[idx] exactly (tail rows through indices >= the ring's capacity), q, da, the BC sum
    and the actor's flat gradient tensor by tensor against fp64."""
    case, nets, dev = _bc_setup(hidden, nh, B, b_demo)
    w = 0.5 if b_demo else 0.0
    o = _actor_rows_bc(nets, dev, B, b_demo, 1.0, w)
    over = _judge_bc(case, nets, o, hidden, nh, B, b_demo, 1.0, w, True)
    assert not over, over


def test_actor_rows_bc_weights_enter_the_gradient(nav):
    """q_weight and bc_weight other than 1 and 0.5 (0.25, 3) at (90, 2, 100, 7)."""
    case, nets, dev = _bc_setup(90, 2, 100, 7)
    o = _actor_rows_bc(nets, dev, 100, 7, 0.25, 3.0)
    over = _judge_bc(case, nets, o, 90, 2, 100, 7, 0.25, 3.0, True)
    assert not over, over


@pytest.mark.parametrize("hidden,nh,B", [(90, 2, 100), (150, 2, BIG)])
def test_actor_rows_bc_off_is_the_plain_form_bit_for_bit(nav, hidden, nh, B):
    """With a critic, q_weight = 1, B_demo = 0 and bc_weight = 0 every output of the BC form
    equals nav_td3_actor_rows' on the same idx (saved rows the launch leaves alone stay NaN in
    both)."""
    case, nets, dev = _bc_setup(hidden, nh, B, 0)
    a = _actor_rows_bc(nets, dev, B, 0, 1.0, 0.0)
    b = _actor_rows_bc(nets, dev, B, 0, 1.0, 0.0, plain=True)
    for key in ("batch", "q", "da", "dz", "acts", "ma", "mc", "es", "g"):
        assert _equal_nan(a[key].float(), b[key].float()), key
    assert bool((a["part"] == 0).all())


BC_ONLY_CASES = [(24, 1, 33), (200, 3, 100), (150, 2, BIG)]


@pytest.mark.parametrize("hidden,nh,B", BC_ONLY_CASES, ids=_ids(BC_ONLY_CASES))
def test_actor_rows_bc_only_vs_fp64(nav, hidden, nh, B):
    """critic = NULL, q = NULL, masks_critic = NULL: da and the flat gradient are the BC term's
    alone (every row a demonstration row, bc_weight 0.5)."""
    case, nets, dev = _bc_setup(hidden, nh, B, B)
    o = _actor_rows_bc(nets, dev, B, B, 1.0, 0.5, critic=False)
    assert bool(o["q"].isnan().all())  # untouched
    over = _judge_bc(case, nets, o, hidden, nh, B, B, 1.0, 0.5, False)
    assert not over, over


# ---- the trainer ----
TRAINER = dict(n_envs=256, envs_per_group=128, hidden=64, n_hidden=2, batch=128,
               updates_per_step=2)


def _learner_state(tr):
    return snapshot(tr, "moments")


@pytest.fixture(scope="module")
def default_run(nav):
    """Three steps of a trainer constructed without the new arguments."""
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, **TRAINER)
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    return tr, _learner_state(tr)


def test_trainer_defaults_change_nothing(nav, default_run):
    """The new arguments at their defaults: parameters, Adam moments and ring bit-identical to a
    trainer constructed without them, no tail, and nav_td3_mix_idx never launched."""
    from nav.trainer import VecTrainer
    ref, want = default_run
    tr = VecTrainer(device=DEV, demo_fraction=0.0, bc_weight=0.0, q_weight=1.0, **TRAINER)
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    assert _same(_learner_state(tr), want)
    assert tr.td3.mix_launches == 0 and ref.td3.mix_launches == 0
    assert tr.replay.tail.shape[0] == 0 and tr.replay.storage.shape == tr.replay.rows.shape
    assert tr.demo_replay is None


def test_trainer_with_demonstrations(nav, default_run, tmp_path):
    """demo_fraction 0.25, bc_weight 1: two constructions agree bit for bit after three steps;
    the ticks leave the tail alone and the ring's bookkeeping is what it is without a tail; the
    tail holds nav_demo_transitions' frame-0 rows of the CEM's demonstrations; save -> load -> one
    more step equals stepping on."""
    from nav.demo_replay import transitions_ref
    from nav.trainer import VecTrainer
    ref, plain = default_run
    runs = []
    for _ in range(2):
        tr = VecTrainer(device=DEV, demo_fraction=0.25, bc_weight=1.0, **TRAINER)
        tail0 = tr.replay.tail.clone()
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        runs.append((tr, tail0))
    (a, tail0), (b, _) = runs
    assert _same(_learner_state(a), _learner_state(b))
    from nav import config as K
    # 2 groups x NUM_DEMO demonstrations x (path length - 1) transitions
    n_tail = 2 * K.NUM_DEMO * (K.DEMOS_CEM_PATH_LENGTH - 1)
    assert tail0.shape == (n_tail, 8) and torch.equal(a.replay.tail, tail0)
    st, ac, gl = a._cem
    assert np.array_equal(tail0.cpu().numpy(), transitions_ref(st.cpu().numpy(), ac.cpu().numpy(),
                                                               gl, 0))
    assert np.array_equal(a.demo_replay.rows1.cpu().numpy(),
                          transitions_ref(st.cpu().numpy(), ac.cpu().numpy(), gl, 1))
    assert (len(a.replay), a.replay.position, a.replay.capacity) == \
        (len(ref.replay), ref.replay.position, ref.replay.capacity)
    assert a.td3.mix_launches == 2 * 3 and a.td3.bc_loss_value() > 0
    assert not torch.equal(a.td3.actor_network.params, plain["actor"])
    path = str(tmp_path / "demo.pt")
    a.save(path)
    c = VecTrainer.load(path, device=DEV)
    assert torch.equal(c.replay.tail, tail0) and c.td3.cfg.demo_fraction == 0.25
    a.step()
    c.step()
    torch.cuda.synchronize()
    assert _same(_learner_state(a), _learner_state(c))


def test_explicit_indices_win_over_the_mix(nav):
    """td3_update(idx_fn=...) with demonstrations on: no mix launch, the BC form runs on the
    given indices (their first B_demo entries address the tail), the reported actor loss is
    the whole L, and two runs agree bit for bit."""
    from nav import config as K
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    B, cap, n_tail = 64, 256, 40
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(cap + n_tail, 8, generator=g) * 10).to(DEV)
    idx = torch.randint(0, cap, (B,), generator=g)
    idx[:16] = cap + torch.randint(0, n_tail, (16,), generator=g)
    idx = idx.to(DEV)
    runs = []
    for _ in range(2):
        cfg = K.TD3Config(batch_size=B, num_epochs=2, demo_fraction=0.25, bc_weight=1.0,
                          net=K.NetConfig(hidden=64, n_hidden=2))
        td3 = TD3(cfg, device=DEV, seed=SEED)
        ring = ReplayRing(cap, DEV, tail=n_tail)
        ring.storage.copy_(rows)
        ring.size = cap
        td3.td3_update(ring, idx_fn=lambda: idx, track_losses=True)
        torch.cuda.synchronize()
        assert td3.mix_launches == 0 and td3.b_demo() == 16
        assert torch.equal(td3.batch2, rows[idx]) and td3.bc_loss_value() > 0
        bc = ((td3.bc_part.double().sum() / 16).item())
        assert abs(td3.actor_losses[-1] - (-(td3.q1.sum() / B).item() + bc)) <= 1e-4 * (1 + bc)
        runs.append(td3.actor_network.params.clone())
    assert torch.equal(*runs)
    with pytest.raises(ValueError):  # a BC weight on a batch without demonstration rows
        TD3(K.TD3Config(batch_size=B, bc_weight=1.0, net=K.NetConfig(hidden=64, n_hidden=2)),
            device=DEV, seed=SEED).td3_update(ring)


def test_pretrain_bc_lowers_the_bc_loss(nav):
    """pretrain_bc(epochs=200, lr=1e-3): bc_loss(frame=1), the loss over every demonstration row
    in order, is strictly lower afterwards; it is deterministic; the target actor is the actor;
    the critics, the ring and the env are untouched and the actor's lr is restored."""
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, **TRAINER)
    assert tr.replay.tail.shape[0] == 0
    before = tr.bc_loss(frame=1)
    assert before == tr.bc_loss(frame=1)
    c1 = tr.td3.critic_network_1.params.clone()
    lr = tr.td3.actor_optimizer.lr
    tr.pretrain_bc(epochs=200, lr=1e-3)
    after = tr.bc_loss(frame=1)
    print(f"bc_loss {before:.6f} -> {after:.6f}")
    assert after < before
    assert torch.equal(tr.td3.target_actor.params, tr.td3.actor_network.params)
    assert torch.equal(tr.td3.critic_network_1.params, c1)
    assert tr.td3.actor_optimizer.lr == lr and tr.td3.cfg.batch_size == TRAINER["batch"]
    assert tr.td3.mix_launches == 200 and tr.steps == 0 and len(tr.replay) == 0
    tr.step()  # training goes on from the cloned actor
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.td3.actor_network.params).all())
